"""Time the draw of readings from the model -- qsc_draw_codes (dense) and qsc_draw_readings (the
sorted readings of a list packing), each also with the refill of the entry arrays that
Observations.resample runs after it -- at the C3 shape and inputs (bench.py's BASELINE recipe:
512 x 512 x 256, R = 8, f = 0.1, seed 20263), with HIP events around replays of captured graphs of
CALLS back-to-back calls (the protocol of tools/bench_check.py: one untimed lead replay, ROUNDS
alternating rounds).  Each draw is set against the HBM time of its algorithmic bytes: dense, the
codes in and out, S once and C; readings, 16 bytes per reading in and out (both sorted arrays read
and written).  Prints one JSON line and writes it to profiles/draw/bench_draw_c3.json.

  python tools/bench_draw.py [--rounds 7] [--out profiles/draw/bench_draw_c3.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quantized_spectrum_cartography_amd import _lib, synthetic  # noqa: E402
from quantized_spectrum_cartography_amd.obs import Observations  # noqa: E402
from tools.bench_check import CALLS, HBM_BYTES_PER_S, SEED, capture, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "draw", "bench_draw_c3.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_draw.py needs an MI355X: nothing is timed without one")
    I, J, K, R = 512, 512, 256, 8
    P = I * J
    prob = synthetic.onebit_problem(I, J, K, R, f=0.1, seed=SEED)
    dense = Observations(prob["Y"], prob["Wx"], prob["b"], prob["sigma"], R_hint=R)
    kk, pp = torch.nonzero(prob["Wx"].reshape(K, P) != 0, as_tuple=True)
    yy = prob["Y"].reshape(K, P)[kk, pp]
    lst = Observations.from_readings(kk, pp // J, pp % J, yy, (K, I, J), prob["b"], prob["sigma"],
                                     R_hint=R)
    n = lst.nnz
    Sd = prob["S0"].reshape(R, -1).float().cuda().contiguous()
    Cd = prob["C0"].float().cuda().contiguous()
    S_pos = lst.to_positions(Sd)
    inv = torch.zeros(1, dtype=torch.int32, device="cuda")
    new_d, new_l = dense.resample(Sd, Cd, seed=1), lst.resample(Sd, Cd, seed=1)
    assert torch.equal(new_d.s_entries, new_l.s_entries)  # one definition, two inputs

    def draw_dense():
        _lib.call("qsc_draw_codes", _lib.ptr(dense.codes), K, P, dense.model, R, _lib.ptr(Sd),
                  _lib.ptr(Cd), 1, 0, _lib.ptr(new_d.codes), _lib.ptr(inv), _lib.stream())

    def draw_readings():
        _lib.call("qsc_draw_readings", _lib.ptr(lst._packed), lst._packed.numel(), n, lst.desc,
                  _lib.ptr(lst.perm), lst.model, R, _lib.ptr(S_pos), _lib.ptr(Cd), 1, 0,
                  _lib.ptr(new_l._packed), _lib.ptr(inv), _lib.stream())

    def refill(o):
        o._fill(o.desc.rowfmt)

    def eager(fn):
        """CALLS back-to-back eager calls (the refill takes its workspace from the caching
        allocator, so it is timed outside a graph: launch gaps included)."""
        def run():
            for _ in range(CALLS):
                fn()
        return run

    runs = {"draw_codes": capture(draw_dense),
            "draw_codes_and_refill": eager(lambda: (draw_dense(), refill(new_d))),
            "draw_readings": capture(draw_readings),
            "draw_readings_and_refill": eager(lambda: (draw_readings(), refill(new_l)))}
    times = {k: [] for k in runs}
    for _ in range(args.rounds):
        for name, run in runs.items():
            times[name].append(timed(run))
    nbytes = {"draw_codes": 2 * K * P + R * P * 4 + R * K * 4, "draw_readings": 16 * n}
    us = {}
    for name, t in times.items():
        st = {"median": statistics.median(t), "min": min(t), "max": max(t),
              "protocol": "graph" if name in nbytes else "eager"}
        if name in nbytes:
            st["hbm_floor_us"] = nbytes[name] / HBM_BYTES_PER_S * 1e6
            st["hbm_roofline_fraction"] = st["hbm_floor_us"] / st["median"]
        us[name] = st
    res = {"shape": {"I": I, "J": J, "K": K, "R": R, "nbins": len(prob["b"]) - 1, "readings": n,
                     "rowfmt": int(dense.desc.rowfmt)},
           "calls_per_graph": CALLS, "rounds": args.rounds, "algorithmic_bytes": nbytes,
           "us_per_call": us}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
