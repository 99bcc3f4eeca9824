"""CPU: the case generator of the fused-pass matrix (tests/test_gpu_pass_matrix.py) and the
conditioning check of its data sets.

The GPU matrix compares every (padded rank, entry type, likelihood kind, log) instantiation of
the fused passes with the fp64 closed forms at the north-star 1e-5.  That margin is meant for
the kernels, so the inputs must not consume it: on every data set the matrix uses, the
reference's own fp32 formulation (oracle.reference_ops.masked_nll / dowjons_cost,
logit_ref.masked_nll, through CPU autograd) has to stay within 3e-6 of the fp64 closed form --
relative NLL, rel_fro(dS), rel_fro(dC).  A data set that misses gets another sigma or seed here;
the tolerances stay.

Shape (the smallest with every edge): 25 x 23 pixels (P = 575, ragged), K = 70 (two k-slices, the
second ragged), tile 128 (Pp = 640: five tiles -- odd, for the snake deal -- and 65 padding
positions), ranks 3, 6, 11 (RP 4, 8, 16, zero pad rows in each), densities 0.3 and 0.03."""
import numpy as np
import pytest
import torch

import logit_ref as lr
from conftest import rel_fro
from oracle import explicit, reference_ops as ro, solver as osolver

I, J, K, TILE = 25, 23, 70, 128
RANKS = (3, 6, 11)
# C-pass form by the tile_parts rule (csrc/qsc_pass_host.cuh), nks = 2, ntiles = 5:
#   chunks = nnz / (ntiles K) / 4 = f 575 / 5 / 4 = 28.75 f 4-entry chunks per bin list and tile;
#   NP starts at 16 / nks = 8 (8 / nks = 4 at rank 16) and drops while chunks / NP < 1.5;
#   the tile form (cpass_tile_kernel) runs when nks NP >= 4, else the per-slice form.
#   f = 0.3:  chunks = 8.6 -> NP = 5 (4 at rank 16) -> 10 (8) units: tile form;
#   f = 0.03: chunks = 0.86 -> NP = 1 -> 2 units: per-slice form (cpass_kernel).
DENSITIES = (0.3, 0.03)
LOG_OFFSET = 1e-3
LOG_FIRST_EDGE = -23.025850296020508  # the reference's first log-model edge, log(1e-10)

# data sets: name -> (bins, log model)
DATASETS = {"lin2": (2, False), "lin5": (5, False), "lin4": (4, False), "log4": (4, True),
            "lin17": (17, False), "log17": (17, True)}

# cells: id -> (kind of the issue's list, loss, data set, entry format, wide)
CELLS = {
    "probit-onebit-sr": ("probit one-bit signed rows", "probit", "lin2", 1, 0),
    "probit-onebit-cf": ("probit one-bit code field", "probit", "lin2", 0, 0),
    "probit-lin": ("probit multi-bin linear", "probit", "lin5", 0, 0),
    "probit-log": ("probit multi-bin log", "probit", "log4", 0, 0),
    "squared-lin": ("squared linear", "squared", "lin4", 0, 0),
    "squared-log": ("squared log", "squared", "log4", 0, 0),
    "logit-onebit-sr": ("logit one-bit signed rows", "logit", "lin2", 1, 0),
    "logit-onebit-cf": ("logit one-bit code field", "logit", "lin2", 0, 0),
    "logit-lin": ("logit multi-bin linear", "logit", "lin5", 0, 0),
    "logit-log": ("logit multi-bin log", "logit", "log4", 0, 0),
    "probit-lin-wide": ("probit multi-bin linear", "probit", "lin17", 0, 1),
    "probit-log-wide": ("probit multi-bin log", "probit", "log17", 0, 1),
    "squared-lin-wide": ("squared linear", "squared", "lin17", 0, 1),
    "squared-log-wide": ("squared log", "squared", "log17", 0, 1),
    "logit-lin-wide": ("logit multi-bin linear", "logit", "lin17", 0, 1),
    "logit-log-wide": ("logit multi-bin log", "logit", "log17", 0, 1),
}

# wide one-bit entries need K or PT above 4096, which only RP 4 can stage (R = 3):
# name -> (I, J, K, tile, f)
WIDE_ONEBIT = {"wide-by-K": (16, 16, 4160, None, 0.05), "wide-by-tile": (65, 64, 20, 4160, 0.3)}

_DATA, _REF, _SOLVE = {}, {}, {}
# data sets whose first seed missed the 3e-6 conditioning bound below (a few improbable entries
# of a sparse pixel carry the fp32 formulation's cancellation into dS: 3.1e-6 .. 1e-5 at the
# log model, mostly at 17 bins and f = 0.03) draw from a later seed: (R, f, data set) -> draw
_RESEED = {(3, 0.3, "log4"): 1, (3, 0.03, "log17"): 5, (6, 0.03, "log17"): 6,
           (11, 0.3, "log17"): 2, (11, 0.03, "log17"): 11}


def make_case(seed, R, I, J, K, f, nbins, log_model):
    """A random problem as tests/test_gpu_fused._random_case draws it; linear boundaries are the
    quantiles of T, log-model boundaries the quantiles of log(T + offset) between the
    reference's first edge and a last edge above the maximum."""
    g = torch.Generator().manual_seed(seed)
    S = torch.rand(R, 1, I, J, generator=g)
    C = torch.rand(R, K, generator=g)
    Tt = ro.get_tensor(S, C)
    q = torch.linspace(0, 1, nbins + 1)
    if log_model:
        off = LOG_OFFSET
        X = torch.log(Tt + off)
        b = torch.quantile(X.reshape(-1)[:100000], q)
        b[0] = LOG_FIRST_EDGE
        b[-1] = float(X.max()) + 1.0
        sigma = (float(X.max()) - float(X.min())) / 4
        Y = ro.quantize(Tt, sigma, b, offset=off, log_model=True,
                        noise=torch.randn(Tt.shape, generator=g))
    else:
        off = 0.0
        b = torch.quantile(Tt.reshape(-1)[:100000], q)
        sigma = (float(Tt.max()) - float(Tt.min())) / 4
        Y = ro.quantize(Tt, sigma, b, noise=torch.randn(Tt.shape, generator=g))
    Wx = torch.bernoulli(torch.full((K, 1, I, J), f), generator=g)
    S0 = 0.5 * torch.rand(R, 1, I, J, generator=g) + (0.25 if log_model else 0.0)
    C0 = 0.5 * torch.rand(R, K, generator=g)
    return dict(Y=Y.unsqueeze(1), Wx=Wx, b=b, sigma=sigma, offset=off, S0=S0, C0=C0,
                log_model=log_model, R=R, I=I, J=J, K=K, nbins=nbins)


def data(R, f, ds):
    """The data set `ds` (DATASETS, or a WIDE_ONEBIT name) at rank R and density f; cached."""
    key = (R, f, ds)
    if key not in _DATA:
        if ds in WIDE_ONEBIT:
            i, j, k, _, f = WIDE_ONEBIT[ds]
            _DATA[key] = make_case(7000 + sorted(WIDE_ONEBIT).index(ds), R, i, j, k, f, 2, False)
        else:
            nbins, log_model = DATASETS[ds]
            seed = 1000 + 100 * R + 10 * DENSITIES.index(f) + sorted(DATASETS).index(ds)
            seed += 10000 * _RESEED.get(key, 0)
            _DATA[key] = make_case(seed, R, I, J, K, f, nbins, log_model)
    return _DATA[key]


def _flat(d):
    R, K, P = d["R"], d["K"], d["I"] * d["J"]
    return (d["S0"].reshape(R, P).numpy(), d["C0"].numpy(), d["Y"].reshape(K, P).numpy(),
            d["Wx"].reshape(K, P).numpy(), d["b"].numpy())


def reference(R, f, ds, loss):
    """(value, dS (R,P), dC (R,K)) of the fp64 closed form, once per data set and loss."""
    key = (R, f, ds, loss)
    if key not in _REF:
        d = data(R, f, ds)
        S, C, Y, Wx, b = _flat(d)
        if loss == "probit":
            r = explicit.nll_grad(S, C, Y, Wx, b, d["sigma"], d["offset"], d["log_model"])
        elif loss == "logit":
            r = lr.nll_grad(S, C, Y, Wx, b, d["sigma"], d["offset"], d["log_model"])
        else:
            r = explicit.sq_loss_grad(S, C, Y, Wx, b, d["offset"], d["log_model"])
        _REF[key] = r
    return _REF[key]


def reference_fp32(R, f, ds, loss):
    """The same three numbers from the reference's fp32 formulation through CPU autograd."""
    d = data(R, f, ds)
    S = d["S0"].clone().requires_grad_(True)
    C = d["C0"].clone().requires_grad_(True)
    if loss == "probit":
        v = ro.masked_nll(S, C, d["Y"], d["Wx"], d["b"], d["sigma"], d["offset"], d["log_model"])
    elif loss == "logit":
        v = lr.masked_nll(S, C, d["Y"], d["Wx"], d["b"], d["sigma"], d["offset"], d["log_model"])
    else:
        v = ro.dowjons_cost(S, C, ro.mid_bin(d["Y"], d["b"]), d["Wx"], d["offset"],
                            d["log_model"])
    v.backward()
    return v.item(), S.grad.reshape(R, -1).numpy(), C.grad.numpy()


SOLVE_ITERS = 3


def solver_reference(R, f, ds, loss):
    """SOLVE_ITERS iterations of the fp32 reference-form free-S solver (default
    hyper-parameters, no projection of S), once per data set and loss."""
    key = (R, f, ds, loss)
    if key not in _SOLVE:
        d = data(R, f, ds)
        a = (d["S0"], d["C0"], d["Y"], d["Wx"], d["b"], d["sigma"])
        kw = dict(offset=d["offset"], log_model=d["log_model"], n_iter=SOLVE_ITERS)
        if loss == "logit":
            _SOLVE[key] = lr.free_s_solve(*a, **kw)
        else:
            _SOLVE[key] = osolver.free_s_solve(*a, loss=loss, project_s=False, **kw)
    return _SOLVE[key]


def errors(got, ref):
    """(relative value error, rel_fro(dS), rel_fro(dC)) of two (value, dS, dC) triples."""
    return (abs(got[0] - ref[0]) / abs(ref[0]), rel_fro(got[1], ref[1]), rel_fro(got[2], ref[2]))


def _conditioning_cases():
    out = []
    for R in RANKS:
        for f in DENSITIES:
            for ds, loss in sorted({(c[2], c[1]) for c in CELLS.values()}):
                out.append(pytest.param(R, f, ds, loss, id="R%d-f%g-%s-%s" % (R, f, ds, loss)))
    for ds in sorted(WIDE_ONEBIT):
        for loss in ("probit", "logit"):
            out.append(pytest.param(3, None, ds, loss, id="R3-%s-%s" % (ds, loss)))
    return out


@pytest.mark.parametrize("R,f,ds,loss", _conditioning_cases())
def test_matrix_data_sets_are_well_conditioned(R, f, ds, loss):
    e = errors(reference_fp32(R, f, ds, loss), reference(R, f, ds, loss))
    print("conditioning R=%d f=%s %s %s: value %.2e dS %.2e dC %.2e" % ((R, f, ds, loss) + e))
    assert max(e) < 3e-6


def test_matrix_data_sets_have_the_intended_edges():
    """Every code of every multi-bin data set occurs among its observed entries (so the 17-bin
    sets reach code 16, past the narrow format's 4-bit field), and the mask is ragged."""
    for R in RANKS:
        for f in DENSITIES:
            for ds, (nbins, _) in DATASETS.items():
                d = data(R, f, ds)
                seen = np.unique(d["Y"][d["Wx"] != 0].numpy())
                assert np.array_equal(seen, np.arange(nbins)), (R, f, ds, seen)
                cnt = d["Wx"].reshape(K, -1).sum(0)
                assert cnt.min() < cnt.max()
