"""Time the subset kernels (qsc_select_codes, qsc_export_codes, qsc_export_readings) and
Observations.split at the C3 shape (bench.py's BASELINE recipe: 512 x 512 x 256, R = 8, f = 0.1,
seed 20263: 6.71 M readings), held-out fraction 0.1.

Kernels: HIP events around replays of captured graphs of CALLS back-to-back calls (one untimed
lead replay, ROUNDS rounds, the median), each set against the HBM time of its algorithmic bytes:
codes in and out for qsc_select_codes; codes in and 9 B per kept reading out for qsc_export_codes
(read twice: the count and the scatter step); 8 B read (two steps of 4) and 9 B written per kept
reading plus the segment table and perm for qsc_export_readings.
End to end: obs.split(0.1) (wall clock, synchronised) for a dense and a list parent against the
host routes it replaces -- qmc.split_holdout plus two constructors, qmc.split_readings plus two
from_readings -- with the run-to-run spread (max - min over the rounds) of each.  Prints one JSON
line and writes it to profiles/select/bench_select_c3.json.

  python tools/bench_select.py [--rounds 7] [--out profiles/select/bench_select_c3.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quantized_spectrum_cartography_amd import _lib, qmc, synthetic  # noqa: E402
from quantized_spectrum_cartography_amd.obs import Observations  # noqa: E402

SEED = 20260 + 3  # bench.py's C3 seed
CALLS = 20
FRAC = 0.1
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


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3  # ms


def stats(t):
    return {"median": statistics.median(t), "min": min(t), "max": max(t), "spread": max(t) - min(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select",
                                                  "bench_select_c3.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_select.py needs an MI355X: nothing is timed without one")
    I, J, K, R = 512, 512, 256, 8
    prob = synthetic.onebit_problem(I, J, K, R, f=FRAC, seed=SEED)
    Y, Wx, b, sigma = prob["Y"], prob["Wx"], prob["b"], prob["sigma"]
    dense = Observations(Y, Wx, b, sigma, R_hint=R)
    kk, ii, jj, cc = (t.clone() for t in dense.readings())
    lst = Observations.from_readings(kk, ii, jj, cc, (K, I, J), b, sigma, R_hint=R,
                                     perm=dense.perm, tile=dense.desc.PT)
    n, P, Pp = dense.nnz, dense.P, dense.Pp
    hi = Observations.frac_range(FRAC)
    p = _lib.ptr
    dev = dense.device
    out = torch.empty_like(dense.codes)
    kept = torch.zeros(1, dtype=torch.int64, device=dev)
    ko = torch.empty(n, dtype=torch.int32, device=dev)
    po = torch.empty(n, dtype=torch.int32, device=dev)
    co = torch.empty(n, dtype=torch.uint8, device=dev)
    no = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(_lib.lib().qsc_export_workspace_bytes(K * P), dtype=torch.uint8, device=dev)
    rule = (None, None, 7, 0, hi, 0)
    tail = (p(ko), p(po), p(co), p(no), p(ws), ws.numel())

    def select_codes():
        _lib.call("qsc_select_codes", p(dense.codes), K, P, *rule, p(out), p(kept), _lib.stream())

    def export_codes():
        _lib.call("qsc_export_codes", p(dense.codes), K, P, *rule, *tail, _lib.stream())

    def export_readings():
        _lib.call("qsc_export_readings", p(lst._packed), lst._packed.numel(), n, lst.desc,
                  p(lst.perm), *rule, *tail, _lib.stream())

    runs = {"select_codes": capture(select_codes), "export_codes": capture(export_codes),
            "export_readings": capture(export_readings)}
    nkept = int(no.item())
    nbytes = {"select_codes": 2 * K * P, "export_codes": 2 * K * P + 9 * nkept,
              "export_readings": 8 * n + 9 * nkept + 2 * 4 * Pp}

    def split_of(o):
        return lambda: o.split(FRAC, seed=7)

    def host_dense():
        Wf, Wh = qmc.split_holdout(Y, Wx, FRAC, 7)
        a = Observations(Y, Wf, b, sigma, R_hint=R)
        Observations(Y, Wh, b, sigma, R_hint=R, tile=a.desc.PT, perm=a.perm)

    def host_list():
        fit, held = qmc.split_readings(n, FRAC, 7)
        f, h = fit.to(dev), held.to(dev)
        a = Observations.from_readings(kk[f], ii[f], jj[f], cc[f], (K, I, J), b, sigma, R_hint=R)
        Observations.from_readings(kk[h], ii[h], jj[h], cc[h], (K, I, J), b, sigma, R_hint=R,
                                   tile=a.desc.PT, perm=a.perm)

    e2e = {"split_dense": split_of(dense), "host_route_dense": host_dense,
           "split_list": split_of(lst), "host_route_list": host_list}
    for fn in e2e.values():
        fn()  # untimed lead (allocator, first-use costs)
    t_us = {k: [] for k in runs}
    t_ms = {k: [] for k in e2e}
    for _ in range(args.rounds):
        for name, run in runs.items():
            t_us[name].append(timed(run))
        for name, fn in e2e.items():
            t_ms[name].append(wall(fn))
    us = {}
    for name, t in t_us.items():
        st = stats(t)
        st["algorithmic_bytes"] = nbytes[name]
        st["hbm_floor_us"] = nbytes[name] / HBM_BYTES_PER_S * 1e6
        st["hbm_roofline_fraction"] = st["hbm_floor_us"] / st["median"]
        us[name] = st
    ms = {name: stats(t) for name, t in t_ms.items()}
    res = {"shape": {"I": I, "J": J, "K": K, "readings": n, "kept_by_the_rule": nkept,
                     "frac": FRAC, "tile": dense.desc.PT},
           "calls_per_graph": CALLS, "rounds": args.rounds, "us_per_call": us,
           "end_to_end_ms": ms,
           "split_over_host_route": {
               f: ms["split_" + f]["median"] / ms["host_route_" + f]["median"]
               for f in ("dense", "list")}}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
