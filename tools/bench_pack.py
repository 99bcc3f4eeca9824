"""Wall time of packing an observation set: the dense path (Observations(Y, Wx): qsc_pack_codes,
qsc_obs_count / _order / _layout / _fill / _schedule) against the readings path
(Observations.from_readings: qsc_obs_readings_count / _layout / _fill, the same order and
schedule calls), in one session.

  python tools/bench_pack.py [--out profiles/readings/bench_pack.json] [--size 512] [--K 256]

Points: C3 (size^2 x K, one-bit, f = 0.1), the same at f = 0.01, and C3 with every reading
given three times (pack time, padding from stats(), fused iteration time next to the
single-reading figure).  The two paths alternate, the device is synchronised around each
packing, and the median of 5 is reported; inputs are on the device for both (the dense path's
int64 Y and fp32 Wx, the readings path's four int64 lists)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from quantized_spectrum_cartography_amd import qmc  # noqa: E402
from quantized_spectrum_cartography_amd.obs import Observations  # noqa: E402

B, SIGMA, R = [-1e5, 0.5, 1e5], 0.25, 8


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def point(N, K, f, reps, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    Y = torch.randint(0, 2, (K, 1, N, N), device="cuda", generator=g)
    Wx = (torch.rand((K, 1, N, N), device="cuda", generator=g) < f).float()
    kk, pp = torch.nonzero(Wx.reshape(K, -1), as_tuple=True)
    o = torch.randperm(kk.numel(), device="cuda", generator=g)  # a list in no useful order
    kk, pp = kk[o], pp[o]
    i, j, c = pp // N, pp % N, Y.reshape(K, -1)[kk, pp]
    dense = lambda: Observations(Y, Wx, B, SIGMA, R_hint=R)  # noqa: E731
    lst = lambda: Observations.from_readings(kk, i, j, c, (K, N, N), B, SIGMA,  # noqa: E731
                                             R_hint=R)
    dense(), lst()  # warm-up: library load, allocator
    td, tr = [], []
    for _ in range(reps):
        t, a = timed(dense)
        td.append(t)
        t, b = timed(lst)
        tr.append(t)
    same = all(torch.equal(getattr(a, n), getattr(b, n))
               for n in ("perm", "s_off", "c_off", "c_kmap", "s_entries", "c_entries"))
    out = dict(N=N, K=K, f=f, readings=int(kk.numel()), dense_ms=[1e3 * x for x in td],
               readings_ms=[1e3 * x for x in tr], dense_median_ms=1e3 * statistics.median(td),
               readings_median_ms=1e3 * statistics.median(tr), bit_identical=bool(same))
    return out, (kk, i, j, c), b


def iter_ms(obs, K, N, iters=100):
    S0 = 0.5 * torch.rand(R, 1, N, N)
    C0 = 0.5 * torch.rand(R, K)
    sol = qmc.FreeSSolver(obs, S0, C0, hist_cap=256)
    sol.run(20)
    t, _ = timed(lambda: sol.run(iters))
    return 1e3 * t / iters, bool(sol.fuse)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--K", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    N, K = a.size, a.K
    res = {"device": torch.cuda.get_device_name(0)}
    res["c3_f0.1"], lists, single = point(N, K, 0.1, a.reps, 1)
    res["c3_f0.01"], _, _ = point(N, K, 0.01, a.reps, 2)
    # every reading three times, the repeats' codes drawn anew
    kk, i, j, c = lists
    g = torch.Generator(device="cuda").manual_seed(3)
    k3, i3, j3 = kk.repeat(3), i.repeat(3), j.repeat(3)
    c3 = torch.cat([c, torch.randint(0, 2, (2 * c.numel(),), device="cuda", generator=g)])
    rep = lambda: Observations.from_readings(k3, i3, j3, c3, (K, N, N), B, SIGMA,  # noqa: E731
                                             R_hint=R)
    rep()
    ts = []
    for _ in range(a.reps):
        t, triple = timed(rep)
        ts.append(t)
    torch.manual_seed(0)
    it1, fused1 = iter_ms(single, K, N)
    it3, fused3 = iter_ms(triple, K, N)
    res["c3_f0.1_x3"] = dict(
        readings=int(k3.numel()), readings_ms=[1e3 * x for x in ts],
        readings_median_ms=1e3 * statistics.median(ts), stats=triple.stats(),
        single_stats=single.stats(), iter_ms=it3, iter_ms_single=it1, fused=fused3,
        fused_single=fused1)
    line = json.dumps(res, indent=1, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
