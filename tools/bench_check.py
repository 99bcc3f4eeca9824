"""Time qsc_scheck (fitted = 0 and fitted = 1) at the C3 shape and inputs (bench.py's BASELINE
recipe: 512 x 512 x 256, R = 8, f = 0.1, seed 20263) with HIP events around replays of captured
graphs of CALLS back-to-back calls (the protocol of tools/bench_design.py: one untimed lead
replay, ROUNDS alternating rounds).  qsc_sinfo (expected kind), which walks the same lists and
evaluates the same bins, is timed alongside as the yardstick.  Each figure is set against the HBM
time of its algorithmic bytes.  Prints one JSON line and writes it to
profiles/check/bench_check_c3.json.

  python tools/bench_check.py [--rounds 7] [--out profiles/check/bench_check_c3.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quantized_spectrum_cartography_amd import fits, qmc, synthetic  # noqa: E402
from quantized_spectrum_cartography_amd.obs import Observations  # noqa: E402

SEED = 20260 + 3  # bench.py's C3 seed
CALLS = 20
HBM_BYTES_PER_S = 6.3e12  # achievable HBM3E rate on MI355X (8 TB/s peak)


def capture(fn):
    """A captured graph of CALLS back-to-back calls of fn (called once eagerly first)."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            for _ in range(CALLS):
                fn()
    torch.cuda.current_stream().wait_stream(s)
    return g.replay


def timed(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    run()  # untimed lead
    e0.record()
    run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / CALLS  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "check",
                                                  "bench_check_c3.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_check.py needs an MI355X: nothing is timed without one")
    I, J, K, R = 512, 512, 256, 8
    prob = synthetic.onebit_problem(I, J, K, R, f=0.1, seed=SEED)
    obs = Observations(prob["Y"], prob["Wx"], prob["b"], prob["sigma"], R_hint=R)
    RP = obs.rank_pad(R)
    Pp = obs.Pp
    S_pos = obs.to_positions(prob["S0"].reshape(R, -1))
    C = prob["C0"].cuda().contiguous()
    ridge = qmc.default_confidence_ridge(prob["S0"], 100.0)
    stat = torch.empty((Pp, 4), dtype=torch.float32, device="cuda")
    count = torch.empty(Pp, dtype=torch.int32, device="cuda")
    flags = torch.empty(Pp, dtype=torch.int32, device="cuda")

    def scheck(fitted):
        fits._check_pos(obs, S_pos, C, R, fitted, ridge, stat, count, flags)

    runs = {"scheck_fitted0": capture(lambda: scheck(False)),
            "scheck_fitted1": capture(lambda: scheck(True)),
            "sinfo_expected": capture(lambda: fits._info_blocks_pos(obs, S_pos, C, R, "expected"))}
    times = {k: [] for k in runs}
    for _ in range(args.rounds):
        for name, run in runs.items():
            times[name].append(timed(run))
    summary = {}
    for fitted in (False, True):
        scheck(fitted)
        torch.cuda.synchronize()
        live = obs.perm >= 0
        summary["fitted%d" % fitted] = {
            "untestable": int(((flags[live] & 1) != 0).sum()),
            "invalid": int(((flags[live] & 2) != 0).sum()),
            "saturated": int(((flags[live] & 4) != 0).sum()),
            "nan": int(torch.isnan(stat).sum()), "entries": int(count.sum())}
    desc, s_entries, _ = obs.layout(R)
    ent_bytes = s_entries.numel() * s_entries.element_size()
    nbytes = ent_bytes + Pp * RP * 4 + Pp * 4 + Pp * 24  # entries, S, perm in; stat, n, flags out
    floor_us = nbytes / HBM_BYTES_PER_S * 1e6
    us = {}
    for name, t in times.items():
        st = {"median": statistics.median(t), "min": min(t), "max": max(t), "protocol": "graph"}
        if name.startswith("scheck"):
            st["hbm_floor_us"] = floor_us
            st["hbm_roofline_fraction"] = floor_us / st["median"]
        us[name] = st
    res = {"shape": {"I": I, "J": J, "K": K, "R": R, "Pp": Pp, "RP": RP,
                     "nbins": len(prob["b"]) - 1, "rowfmt": int(desc.rowfmt)},
           "calls_per_graph": CALLS, "rounds": args.rounds, "ridge": ridge,
           "algorithmic_bytes": {"entries": ent_bytes, "S": Pp * RP * 4, "perm": Pp * 4,
                                 "out": Pp * 24, "scheck": nbytes},
           "counts": summary, "us_per_call": us}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
