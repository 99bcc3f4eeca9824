"""Time the Fisher-information kernels, qsc_sinfo (both kinds) and qsc_info_std (with and without
the map's standard deviations), at the C3 shape and inputs (bench.py's BASELINE recipe:
512 x 512 x 256, R = 8, f = 0.1, seed 20263), with HIP events around replays of captured graphs of
CALLS back-to-back calls (the protocol of tools/bench_smooth.py: one untimed lead replay, ROUNDS
alternating rounds), and set each against the HBM time of its algorithmic bytes (DESIGN.md section
7k).  Prints one JSON line and writes it to profiles/info/bench_info_c3.json.

  python tools/bench_info.py [--rounds 7] [--out profiles/info/bench_info_c3.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quantized_spectrum_cartography_amd import _lib, qmc, synthetic  # noqa: E402
from quantized_spectrum_cartography_amd.obs import Observations  # noqa: E402

SEED = 20260 + 3  # bench.py's C3 seed
CALLS = 50
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
    return g


def timed_graph(g):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    g.replay()  # untimed lead
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / CALLS  # us per call


def stats(t, floor_us):
    st = {"median": statistics.median(t), "min": min(t), "max": max(t), "hbm_floor_us": floor_us}
    st["hbm_roofline_fraction"] = floor_us / st["median"]
    return st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "info", "bench_info_c3.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_info.py needs an MI355X: nothing is timed without one")
    I, J, K, R = 512, 512, 256, 8
    prob = synthetic.onebit_problem(I, J, K, R, f=0.1, seed=SEED)
    obs = Observations(prob["Y"], prob["Wx"], prob["b"], prob["sigma"], R_hint=R)
    desc, s_entries, _ = obs.layout(R)
    RP = obs.rank_pad(R)
    Pp, P = obs.Pp, obs.P
    S_pos = obs.to_positions(prob["S0"].reshape(R, -1))
    C = prob["C0"].cuda().contiguous()
    Jb = torch.empty((Pp, RP, RP), dtype=torch.float32, device="cuda")
    std = torch.empty((Pp, RP), dtype=torch.float32, device="cuda")
    std_T = torch.empty((K, P), dtype=torch.float32, device="cuda")
    nbad = torch.zeros(1, dtype=torch.int32, device="cuda")
    ridge = qmc.default_confidence_ridge(prob["S0"], 100.0)
    p = _lib.ptr

    def sinfo(kind):
        _lib.call("qsc_sinfo", desc, p(s_entries), p(obs.s_width), p(obs.s_off), obs.model, R,
                  p(S_pos), p(C), qmc.INFO_KINDS[kind], p(Jb), _lib.stream())

    def info_std(with_map):
        _lib.call("qsc_info_std", p(Jb), p(obs.perm), R, P, Pp, p(C), K, ridge, p(std),
                  p(std_T) if with_map else None, p(nbad), _lib.stream())

    ent_bytes = int(desc.s_entries) * obs.entry_bytes
    s_bytes, j_bytes = Pp * RP * 4, Pp * RP * RP * 4
    nbytes = {"sinfo": ent_bytes + s_bytes + j_bytes,
              "info_std": j_bytes + Pp * 4 + Pp * RP * 4,
              "info_std_map": j_bytes + Pp * 4 + Pp * RP * 4 + K * P * 4}
    graphs = {"sinfo_expected": (capture(lambda: sinfo("expected")), "sinfo"),
              "sinfo_observed": (capture(lambda: sinfo("observed")), "sinfo")}
    sinfo("expected")  # the blocks the factorisations are timed on
    graphs["info_std"] = (capture(lambda: info_std(False)), "info_std")
    graphs["info_std_map"] = (capture(lambda: info_std(True)), "info_std_map")
    times = {k: [] for k in graphs}
    for _ in range(args.rounds):
        for name, (g, _) in graphs.items():
            times[name].append(timed_graph(g))
    nbad.zero_()
    info_std(False)
    torch.cuda.synchronize()
    out = {"shape": {"I": I, "J": J, "K": K, "R": R, "Pp": Pp, "RP": RP, "nnz": int(obs.nnz),
                     "s_entries": int(desc.s_entries), "entry_bytes": obs.entry_bytes,
                     "rowfmt": int(desc.rowfmt)},
           "calls_per_graph": CALLS, "rounds": args.rounds, "ridge": ridge,
           "unidentified": int(nbad.item()),
           "algorithmic_bytes": {"entries": ent_bytes, "S": s_bytes, "blocks": j_bytes, **nbytes},
           "us_per_call": {name: stats(t, nbytes[key] / HBM_BYTES_PER_S * 1e6)
                           for (name, (_, key)), t in zip(graphs.items(), times.values())}}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
