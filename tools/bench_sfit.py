"""Time the per-pixel Newton fit qsc_sfit at the C3 shape and inputs (bench.py's BASELINE recipe:
512 x 512 x 256, R = 8, f = 0.1, seed 20263) with the C of a standard solver run, with HIP events
around replays of captured graphs of CALLS back-to-back calls (the protocol of tools/bench_info.py:
one untimed lead replay, ROUNDS alternating rounds).

  (a) the time of one walk-and-solve iteration, by differencing max_steps = 1 and 3 with a
      tolerance no step meets (so that no wave leaves early), against qsc_sinfo's observed-kind
      call in the same session (the same walk, writing the blocks);
  (b) the full fit_S from S = 0 with the defaults: the histogram of steps and the total time.
The Adam comparator (S-steps with C frozen to the same objective) is not measured here.
Prints one JSON line and writes it to profiles/sfit/bench_sfit_c3.json.

  python tools/bench_sfit.py [--rounds 7] [--iters 200] [--out profiles/sfit/bench_sfit_c3.json]
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
CALLS = 10


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200, help="solver iterations that produce C")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sfit", "bench_sfit_c3.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sfit.py needs an MI355X: nothing is timed without one")
    I, J, K, R = 512, 512, 256, 8
    prob = synthetic.onebit_problem(I, J, K, R, f=0.1, seed=SEED)
    obs = Observations(prob["Y"], prob["Wx"], prob["b"], prob["sigma"], R_hint=R)
    sol = qmc.FreeSSolver(obs, prob["S0"], prob["C0"])
    sol.run(args.iters)
    torch.cuda.synchronize()
    C = sol.C.clone()
    ridge = qmc.default_confidence_ridge(sol.S_pixels(), 100.0)
    desc, s_entries, _ = obs.layout(R)
    RP, Pp = obs.rank_pad(R), obs.Pp
    S0 = torch.zeros((Pp, RP), dtype=torch.float32, device="cuda")
    S_out = torch.empty_like(S0)
    Jb = torch.empty((Pp, RP, RP), dtype=torch.float32, device="cuda")
    p = _lib.ptr

    def sinfo():
        _lib.call("qsc_sinfo", desc, p(s_entries), p(obs.s_width), p(obs.s_off), obs.model, R,
                  p(sol.S), p(C), qmc.INFO_KINDS["observed"], p(Jb), _lib.stream())

    def sfit(max_steps, tol):
        qmc._fit_s_pos(obs, S0, C, R, "observed", ridge, max_steps, tol, 1e-3, False, S_out=S_out)

    graphs = {"sinfo_observed": capture(sinfo),
              "sfit_steps1": capture(lambda: sfit(1, 1e-30)),
              "sfit_steps3": capture(lambda: sfit(3, 1e-30)),
              "sfit_full": capture(lambda: sfit(30, 1e-5))}
    times = {k: [] for k in graphs}
    for _ in range(args.rounds):
        for name, g in graphs.items():
            times[name].append(timed_graph(g))
    med = {k: statistics.median(v) for k, v in times.items()}
    res = qmc.fit_S(obs, C, ridge=ridge)
    hist = torch.bincount(res.steps.reshape(-1).long()).tolist()
    per_iter = (med["sfit_steps3"] - med["sfit_steps1"]) / 2.0
    out = {"shape": {"I": I, "J": J, "K": K, "R": R, "Pp": Pp, "RP": RP, "nnz": int(obs.nnz),
                     "s_entries": int(desc.s_entries), "rowfmt": int(desc.rowfmt)},
           "solver_iters_for_C": args.iters, "ridge": ridge, "calls_per_graph": CALLS,
           "rounds": args.rounds,
           "us_per_call": {k: {"median": med[k], "min": min(v), "max": max(v)}
                           for k, v in times.items()},
           "us_per_iteration": per_iter,
           "iteration_over_sinfo_observed": per_iter / med["sinfo_observed"],
           "full_fit": {"us": med["sfit_full"], "steps_histogram": hist, "nll": res.nll,
                        "unconverged": res.unconverged, "unidentified": res.unidentified}}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
