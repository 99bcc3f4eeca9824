"""Time the captured free-S iteration under loss="logit" against loss="probit" on one build, at
the C3 shape and inputs (bench.py's BASELINE recipe: 512 x 512 x 256, R = 8, f = 0.1, seed
20263; the same Y, mask and starting point for both), with HIP events on the replay stream;
prints one JSON line.

Both solvers are built and warmed first; then ROUNDS rounds alternate the two (probit, logit,
probit, ...), each round one prepared hipGraph replay of ITERS outer iterations (2 x ITERS
grad-steps) behind LEAD untimed iterations, as bench.py's timed_run does.  The figures are the
medians over the rounds; the spread (min / max) is printed with them.

  python tools/bench_logit.py [--iters 200] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantized_spectrum_cartography_amd import synthetic  # noqa: E402
from quantized_spectrum_cartography_amd.obs import Observations  # noqa: E402
from quantized_spectrum_cartography_amd.qmc import FreeSSolver  # noqa: E402

SEED = 20260 + 3  # bench.py's C3 seed
LEAD = 8


def timed(sol, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    sol.run(LEAD, use_graph=True)  # untimed: runs while the host submits the timed replay
    e0.record()
    sol.run(iters, use_graph=True)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us per outer iteration


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_logit.py needs an MI355X: nothing is timed without one")
    I, J, K, R = 512, 512, 256, 8
    prob = synthetic.onebit_problem(I, J, K, R, f=0.1, seed=SEED)
    sols = {}
    for loss in ("probit", "logit"):
        obs = Observations(prob["Y"], prob["Wx"], prob["b"], prob["sigma"], R_hint=R, loss=loss)
        sol = FreeSSolver(obs, prob["S0"], prob["C0"])
        assert sol.fuse and obs.desc.rowfmt == 1
        sol.run(4, use_graph=True)
        sol.prepare(args.iters)
        sol.prepare(LEAD)
        sols[loss] = sol
    times = {k: [] for k in sols}
    for _ in range(args.rounds):
        for loss, sol in sols.items():
            times[loss].append(timed(sol, args.iters))
    out = {"shape": {"I": I, "J": J, "K": K, "R": R, "nnz": int(sols["probit"].obs.nnz)},
           "iters_per_round": args.iters, "rounds": args.rounds}
    for loss, t in times.items():
        med = statistics.median(t)
        out[loss] = {"us_per_iter_median": med, "us_per_iter_min": min(t), "us_per_iter_max": max(t),
                     "grad_steps_per_s": 2e6 / med}
    out["logit_over_probit_time"] = (out["logit"]["us_per_iter_median"] /
                                     out["probit"]["us_per_iter_median"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
