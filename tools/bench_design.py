"""Time qsc_sgain (criteria D and V) at the C3 shape and inputs (bench.py's BASELINE recipe:
512 x 512 x 256, R = 8, f = 0.1, seed 20263) against the composition from torch ops and existing
entry points that it replaces -- the map T = C^T S (K x P), its per-entry expected information
(qsc_entry_info, K x P), the [P, K] x [K, R^2] product that forms A, and two batched Choleskys --
with HIP events around replays of captured graphs of CALLS back-to-back calls (the protocol of
tools/bench_info.py: one untimed lead replay, ROUNDS alternating rounds).  Where the composition
cannot be captured into a graph (a library call that synchronises), it is timed as CALLS eager
back-to-back calls between two events instead, and the output says so.  Each fused figure is set
against the HBM time of its algorithmic bytes.  Prints one JSON line and
writes it to profiles/design/bench_design_c3.json.

  python tools/bench_design.py [--rounds 7] [--out profiles/design/bench_design_c3.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quantized_spectrum_cartography_amd import _lib, fits, qmc, synthetic  # noqa: E402
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


def eager(fn):
    def run():
        for _ in range(CALLS):
            fn()
    return run


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "design",
                                                  "bench_design_c3.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_design.py needs an MI355X: nothing is timed without one")
    I, J, K, R = 512, 512, 256, 8
    prob = synthetic.onebit_problem(I, J, K, R, f=0.1, seed=SEED)
    obs = Observations(prob["Y"], prob["Wx"], prob["b"], prob["sigma"], R_hint=R)
    RP = obs.rank_pad(R)
    Pp, P = obs.Pp, obs.P
    S_pos = obs.to_positions(prob["S0"].reshape(R, -1))
    C = prob["C0"].cuda().contiguous()
    ridge = qmc.default_confidence_ridge(prob["S0"], 100.0)
    Jb = fits._info_blocks_pos(obs, S_pos, C, R, "expected")
    G = torch.zeros((RP, RP), device="cuda")
    G[:R, :R] = C @ C.t()
    gain = torch.empty(Pp, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    p = _lib.ptr

    def sgain(crit):
        _lib.call("qsc_sgain", p(S_pos), p(C), p(Jb), p(obs.perm), None, p(G), obs.model, R, K, P,
                  Pp, qmc.DESIGN_CRITERIA[crit], ridge, p(gain), p(cnt[0:1]), p(cnt[1:2]),
                  _lib.stream())

    # ---- the composition: position order throughout, so no gather is charged to it ----
    S_rp = S_pos[:, :R].contiguous()                       # (Pp, R)
    J0 = Jb[:, :R, :R].contiguous() + ridge * torch.eye(R, device="cuda")
    CC = (C.t()[:, :, None] * C.t()[:, None, :]).reshape(K, R * R).contiguous()  # vec(c_k c_k^T)
    Yz = torch.zeros((Pp, K), dtype=torch.int64, device="cuda")
    H = torch.empty((Pp, K), dtype=torch.float32, device="cuda")
    Gr = G[:R, :R].contiguous()
    out = {}

    def composed(crit):
        T = S_rp @ C                                       # (Pp, K): the map
        _lib.call("qsc_entry_info", p(Yz), p(T), T.numel(), obs.model,
                  qmc.INFO_KINDS["expected"], p(H), _lib.stream())
        A = (H @ CC).reshape(Pp, R, R)                     # [P, K] x [K, R^2]
        L0, _ = torch.linalg.cholesky_ex(J0)
        L1, _ = torch.linalg.cholesky_ex(J0 + A)
        if crit == "D":
            out[crit] = (torch.log(torch.diagonal(L1, dim1=1, dim2=2)).sum(1)
                         - torch.log(torch.diagonal(L0, dim1=1, dim2=2)).sum(1))
        else:
            X0 = torch.cholesky_inverse(L0)
            X1 = torch.cholesky_inverse(L1)
            out[crit] = ((X0 - X1) * Gr).sum((1, 2))      # tr(G M0^-1) - tr(G M1^-1)
        out["A"] = A

    runs, protocol = {}, {}
    for crit in ("D", "V"):
        runs["sgain_" + crit] = capture(lambda c=crit: sgain(c))
        protocol["sgain_" + crit] = "graph"
        name = "composed_" + crit
        try:
            runs[name] = capture(lambda c=crit: composed(c))
            protocol[name] = "graph"
        except Exception as e:  # a synchronising library call inside the capture
            torch.cuda.synchronize()
            composed(crit)
            runs[name] = eager(lambda c=crit: composed(c))
            protocol[name] = "eager (%s)" % type(e).__name__
    times = {k: [] for k in runs}
    for _ in range(args.rounds):
        for name, run in runs.items():
            times[name].append(timed(run))
    # the two agree (identified positions; the composition knows no padding or first looks), and
    # both agree with an fp64 evaluation on the host at a sample of positions
    agree, vs64 = {}, {}
    live = (obs.perm >= 0)
    sample = torch.nonzero(live).reshape(-1)[::4099][:64]
    for crit in ("D", "V"):
        cnt.zero_()
        sgain(crit)
        composed(crit)
        a, b = gain[live].double(), out[crit][live].double()
        ok = torch.isfinite(a) & torch.isfinite(b)
        agree[crit] = float((a[ok] - b[ok]).abs().max() / b[ok].abs().max())
        M0 = J0[sample].double().cpu()
        M1 = M0 + out["A"][sample].double().cpu()
        if crit == "D":
            ref = 0.5 * (torch.linalg.slogdet(M1)[1] - torch.linalg.slogdet(M0)[1])
        else:
            G64 = Gr.double().cpu()
            ref = ((torch.linalg.inv(M0) - torch.linalg.inv(M1)) * G64).sum((1, 2))
        vs64[crit] = {"sgain": float((gain[sample].double().cpu() - ref).abs().max()
                                     / ref.abs().max()),
                      "composed": float((out[crit][sample].double().cpu() - ref).abs().max()
                                        / ref.abs().max())}
    torch.cuda.synchronize()
    s_bytes, j_bytes = Pp * RP * 4, Pp * RP * RP * 4
    nbytes = s_bytes + j_bytes + Pp * 4 + Pp * 4  # S, J, perm in; gain out
    floor_us = nbytes / HBM_BYTES_PER_S * 1e6
    us = {}
    for name, t in times.items():
        st = {"median": statistics.median(t), "min": min(t), "max": max(t),
              "protocol": protocol[name]}
        if name.startswith("sgain"):
            st["hbm_floor_us"] = floor_us
            st["hbm_roofline_fraction"] = floor_us / st["median"]
        us[name] = st
    res = {"shape": {"I": I, "J": J, "K": K, "R": R, "Pp": Pp, "RP": RP,
                     "nbins": len(prob["b"]) - 1},
           "calls_per_graph": CALLS, "rounds": args.rounds, "ridge": ridge,
           "first_look": int(cnt[0].item()), "degenerate": int(cnt[1].item()),
           "algorithmic_bytes": {"S": s_bytes, "blocks": j_bytes, "perm": Pp * 4, "gain": Pp * 4,
                                 "sgain": nbytes,
                                 "composition_map_and_information": 2 * Pp * K * 4},
           "link_evaluations_per_call": Pp * K * (len(prob["b"]) - 1),
           "max_rel_difference_fused_vs_composed": agree,
           "max_rel_difference_vs_fp64_at_64_positions": vs64,
           "us_per_call": us,
           "speedup_median": {c: us["composed_" + c]["median"] / us["sgain_" + c]["median"]
                              for c in ("D", "V")}}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
