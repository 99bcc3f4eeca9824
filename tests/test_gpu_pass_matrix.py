"""GPU: every instantiation of the fused passes (QSC_DISPATCH_PASS, csrc/qsc_pass_host.cuh:
padded rank 4 / 8 / 16 x narrow / wide entries x likelihood kind x log) against independent
references, on the smallest shape that has every edge (tests/test_pass_matrix_host.py: 25 x 23
pixels, K = 70, tile 128, ranks 3 / 6 / 11, densities 0.3 -- tile-form C-pass -- and 0.03 --
per-slice C-pass).

1. fused.ProbitNLL.apply (qsc_spass mode 0, qsc_cpass, qsc_cfinish mode 0) against the fp64 closed
   forms (oracle.explicit.nll_grad / sq_loss_grad, logit_ref.nll_grad);
2. three iterations of qmc.solve (qsc_spass mode 1, qsc_cfinish mode 1, qsc_scpass; unfused,
   fused, fused through a hipGraph) against the fp32 reference-form solver;
3. a configuration the library cannot run is refused before any launch.

Tolerance: the project's north-star 1e-5 throughout (relative value, rel_fro of gradients and of
S, C, relative cost histories).  The data sets are conditioned so that the reference's own fp32
formulation is within 3e-6 of fp64 (asserted on the CPU in test_pass_matrix_host.py)."""
import numpy as np
import pytest

from conftest import rel_fro
from test_pass_matrix_host import (CELLS, DENSITIES, RANKS, SOLVE_ITERS, TILE, WIDE_ONEBIT, data,
                                   errors, reference, solver_reference)

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _observations(d, R, tile, loss):
    from quantized_spectrum_cartography_amd.obs import Observations
    return Observations(d["Y"], d["Wx"], d["b"], d["sigma"], offset=d["offset"],
                        log_model=d["log_model"], R_hint=R, tile=tile, loss=loss)


def _cell_obs(cell, R, f):
    """The packed observations of a matrix cell, with the layout facts the cell is about."""
    _, loss, ds, fmt, wide = CELLS[cell]
    d = data(R, f, ds)
    obs = _observations(d, R, TILE, loss)
    dsc = obs.desc
    assert (dsc.PT, dsc.Pp, dsc.ntiles, dsc.nks) == (TILE, 640, 5, 2)
    assert obs.nnz == int(d["Wx"].sum())
    assert dsc.wide == wide
    onebit = d["nbins"] == 2
    assert dsc.rowfmt == (1 if onebit else 0)
    if onebit and fmt == 0:
        obs._fill(0)
    assert dsc.rowfmt == fmt
    if wide:  # every code 0..16 is observed: codes past the narrow 4-bit field are in play
        codes = obs.codes.cpu().numpy()
        assert np.array_equal(np.unique(codes[codes != 0xFF]), np.arange(17))
    return d, obs, loss, ds


def _pass(d, obs, R):
    from quantized_spectrum_cartography_amd import fused
    S = d["S0"].cuda().requires_grad_(True)
    C = d["C0"].cuda().requires_grad_(True)
    v = fused.ProbitNLL.apply(S, C, obs)
    v.backward()
    return v.item(), S.grad.cpu().reshape(R, -1).numpy(), C.grad.cpu().numpy()


@pytest.mark.parametrize("f", DENSITIES)
@pytest.mark.parametrize("R", RANKS)
@pytest.mark.parametrize("cell", sorted(CELLS))
def test_pass_matrix_vs_fp64(cell, R, f):
    d, obs, loss, ds = _cell_obs(cell, R, f)
    e = errors(_pass(d, obs, R), reference(R, f, ds, loss))
    print("pass %s R=%d f=%g wide=%d rowfmt=%d: value %.2e dS %.2e dC %.2e"
          % ((cell, R, f, obs.desc.wide, obs.desc.rowfmt) + e))
    assert e[0] < TOL
    assert e[1] < TOL
    assert e[2] < TOL


@pytest.mark.parametrize("loss", ["probit", "logit"])
@pytest.mark.parametrize("ds", sorted(WIDE_ONEBIT))
def test_pass_wide_onebit_vs_fp64(ds, loss):
    """Wide one-bit entries (K or the tile above 4096; only RP 4 can stage such tables)."""
    d = data(3, None, ds)
    obs = _observations(d, 3, WIDE_ONEBIT[ds][3], loss)
    assert obs.desc.wide == 1 and obs.desc.rowfmt == 0
    e = errors(_pass(d, obs, 3), reference(3, None, ds, loss))
    print("pass %s-%s R=3 wide=1 rowfmt=0: value %.2e dS %.2e dC %.2e" % ((ds, loss) + e))
    assert e[0] < TOL
    assert e[1] < TOL
    assert e[2] < TOL


def _relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def _solver_checks(tag, d, obs, loss, ref, expect_fused=None):
    from quantized_spectrum_cartography_amd import qmc
    from quantized_spectrum_cartography_amd.fused import PassEngine
    R = d["R"]
    supported = PassEngine(obs, R).scpass_supported()
    if expect_fused is not None:
        assert supported == expect_fused
    kw = dict(S_init=d["S0"], C_init=d["C0"], max_iter=SOLVE_ITERS, obs=obs, project_s=False)
    runs = [qmc.solve(d["Y"], d["Wx"], d["b"], d["sigma"], fuse=False, **kw),
            qmc.solve(d["Y"], d["Wx"], d["b"], d["sigma"], fuse=True, **kw),
            qmc.solve(d["Y"], d["Wx"], d["b"], d["sigma"], fuse=True, use_graph=True, **kw)]
    a = runs[0]
    assert not a.fused
    e = (rel_fro(a.S.cpu().numpy(), ref["S"].numpy()), rel_fro(a.C.cpu().numpy(), ref["C"].numpy()),
         _relmax(a.costs_c, ref["costs_c"]), _relmax(a.costs_s, ref["costs_s"]))
    print("solve %s fused=%d: S %.2e C %.2e costs_c %.2e costs_s %.2e" % ((tag, supported) + e))
    assert len(a.costs_c) == len(a.costs_s) == SOLVE_ITERS
    assert e[0] < TOL
    assert e[1] < TOL
    assert e[2] < TOL
    assert e[3] < TOL
    for b in runs[1:]:
        assert b.fused == supported
        assert np.array_equal(a.S.cpu().numpy(), b.S.cpu().numpy())
        assert np.array_equal(a.C.cpu().numpy(), b.C.cpu().numpy())
        assert a.costs_c == b.costs_c and a.costs_s == b.costs_s


def _solver_cells():
    """Every wide cell, the narrow multi-bin cells at R = 6 and 11, and the probit and squared
    ones at R = 3."""
    out = []
    for cell in sorted(CELLS):
        _, loss, ds, _, wide = CELLS[cell]
        if ds == "lin2":
            continue
        for R in RANKS:
            if wide or R > 3 or loss != "logit":
                out.append((cell, R))
    return out


@pytest.mark.parametrize("f", DENSITIES)
@pytest.mark.parametrize("cell,R", _solver_cells())
def test_solver_matrix_vs_reference(cell, R, f):
    d, obs, loss, ds = _cell_obs(cell, R, f)
    # the fused launch applies to every cell of this shape (its C-pass units and LDS fit)
    _solver_checks("%s R=%d f=%g" % (cell, R, f), d, obs, loss, solver_reference(R, f, ds, loss),
                   expect_fused=True)


@pytest.mark.parametrize("loss", ["probit", "logit"])
@pytest.mark.parametrize("ds", sorted(WIDE_ONEBIT))
def test_solver_wide_onebit_vs_reference(ds, loss):
    d = data(3, None, ds)
    obs = _observations(d, 3, WIDE_ONEBIT[ds][3], loss)
    assert obs.desc.wide == 1 and obs.desc.rowfmt == 0
    # the fused launch needs PT <= 4096 and at most 16 C-pass units per tile (K = 4160: 65)
    _solver_checks("%s-%s R=3" % (ds, loss), d, obs, loss, solver_reference(3, None, ds, loss),
                   expect_fused=False)


def test_unrunnable_rank_is_refused_before_any_launch():
    """R = 6 at K = 4160: the S-pass table [K][RP + 4] needs 200 KB of LDS, over the 160 KB of
    a workgroup; qsc_spass returns QSC_EINVAL from its argument checks, ahead of its launch.  The
    Python layer raises its library error, and the stream goes on giving the oracle's results."""
    from quantized_spectrum_cartography_amd import _lib, fused
    d = data(6, None, "wide-by-K")
    obs = _observations(d, 6, None, "probit")
    assert obs.desc.wide == 1 and obs.desc.rowfmt == 0
    S = d["S0"].cuda().requires_grad_(True)
    C = d["C0"].cuda()  # (no dC wanted: the S-pass is the only pass this call issues)
    with pytest.raises(_lib.QscError, match="qsc_spass"):
        fused.ProbitNLL.apply(S, C, obs)
    cell = "probit-lin"
    small, sobs, loss, ds = _cell_obs(cell, 6, 0.3)
    e = errors(_pass(small, sobs, 6), reference(6, 0.3, ds, loss))
    assert max(e) < TOL
