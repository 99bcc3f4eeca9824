"""CPU: the conditions tests/test_gpu_list_matrix.py rests on, from the references alone
(tests/list_matrix_ref.py has the matrix, the mask and the reasoning).

1. CELLS is the full product rank x link x data set, and every cell's model is one the list
   kernels' layout check admits.
2. Every cell's mask has pixel 0 empty, the 1 .. 5 ladder, the full pixel and both end bins, and
   every code of the model among its observed entries (the 16-bin sets reach code 15, the narrow
   format's pad code).
3. Floor: for every cell, kind and stepped quantity (qsc_sfit at both ridges, qsc_cfit at both
   ridges, one qsc_sfit_smooth visit of each colour and prior kind) the fp32 numpy reference is
   within 1e-4 of the fp64 one in the per-pixel norm, over the compared set.  A cell that misses
   gets other inputs in list_matrix_ref.py (sigma, the start); the cap stays.
4. Accept decisions: the pixels (bins) where fp32 and fp64 disagree are at most 10 % of a cell's,
   and at least a quarter of the compared ones accept their step in fp64 -- a rejected step compares
   the start with itself and would test nothing.
5. The 16-bin logit finding (list_matrix_ref.py's docstring): the observed curvature is positive
   and equals the finite difference of the score, the undamped step from 0.8 S_true overshoots,
   and from START it is accepted.
"""
import numpy as np
import pytest

import check_ref as ckr
import info_ref as ir
import list_matrix_ref as lm
import sfit_ref as sr
import sfit_smooth_ref as ssr

CELL_IDS = sorted(lm.CELLS)
SMOOTH_RIDGE = 1e-2
CHECK_RIDGE = 1.0  # (at 1e-2 the log model's I* / Ixx sits inside the guard's window)


def test_cells_are_the_full_product():
    want = {(R, loss, ds) for R in (3, 6, 11) for loss in ("probit", "logit")
            for ds in ("narrow-lin", "narrow-log", "wide-lin", "wide-log", "signed")}
    assert len(want) == 30 and len(lm.CELLS) == 30
    assert set(lm.CELLS.values()) == want
    assert all(lm.cell_id(*v) == k for k, v in lm.CELLS.items())
    pads = {(lm.RANK_PAD[R], lm.DATASETS[ds][3], lm.DATASETS[ds][2], loss, lm.DATASETS[ds][1])
            for R, loss, ds in lm.CELLS.values()}
    # rank pad x (wide, signed rows) x link x log, without signed rows under the log model
    assert len(pads) == 30
    assert {p[0] for p in pads} == {4, 8, 16}


@pytest.mark.parametrize("cell", CELL_IDS)
def test_cell_model_mask_and_codes(cell):
    d = lm.problem(cell)
    R, K = d["R"], d["K"]
    assert lm.layout_rules(d)
    assert K == (37 if R == 3 else 70) and d["RP"] == {3: 4, 6: 8, 11: 16}[R]
    assert bool(d["wide"]) == (d["nbins"] > 15) and bool(d["rowfmt"]) == (d["nbins"] == 2)
    W = d["Wx"].reshape(K, lm.P).numpy() != 0
    cnt = W.sum(axis=0)
    assert cnt[0] == 0
    assert [int(cnt[n]) for n in lm.LADDER] == [1, 2, 3, 4, 5]
    assert cnt[lm.FULL_PIXEL] == K
    assert W[K - 1, 1] and W[0, 2] and W[K - 1, 2]
    assert W[0].any() and W[K - 1].any() and W.any(axis=1).all()
    rest = cnt[lm.FULL_PIXEL + 1:]
    assert rest.min() > 5 and rest.max() < K and 0.6 < rest.mean() / K < 0.8
    seen = np.unique(d["Y"].reshape(K, lm.P).numpy()[W])
    assert np.array_equal(seen, np.arange(d["nbins"]))
    # the map stays inside the log model's domain at the truth and at the start
    S, C = lm.flat(d)
    assert (C.T @ S).min() > 0 and (C.T @ lm.s_start(d)).min() > 0


def _report(what, cell, kind, extra, n, keep, acc, floor):
    print("lm-host %s %s %s %s: of %d disagree %d accepted %d floor %.2e"
          % (what, cell, kind, extra, n, n - int(keep.sum()), int(acc.sum()), floor))


def _conditions(n, keep, acc, floor):
    assert n - int(keep.sum()) <= lm.MAX_DISAGREE * n
    assert int(acc.sum()) >= lm.MIN_ACCEPTED * int(keep.sum())
    assert floor <= lm.FLOOR_CAP


@pytest.mark.parametrize("kind", lm.KINDS)
@pytest.mark.parametrize("cell", CELL_IDS)
def test_step_floors_and_accept_decisions(cell, kind):
    d = lm.problem(cell)
    op, ob = lm.observed_pixels(d), lm.observed_bins(d)
    assert op.sum() == lm.P - 1 and ob.all()
    for ridge in lm.RIDGES:
        r64, r32 = (lm.sfit_step(cell, kind, ridge, t) for t in (np.float64, np.float32))
        keep, acc = lm.compared(r64, r32, lm.s_start(d), op)
        floor = lm.pixel_rel(r32["S"], r64["S"], keep)
        _report("sfit", cell, kind, "ridge %g" % ridge, int(op.sum()), keep, acc, floor)
        _conditions(int(op.sum()), keep, acc, floor)
        r64, r32 = (lm.cfit_step(cell, kind, ridge, t) for t in (np.float64, np.float32))
        keep, acc = lm.compared(r64, r32, lm.c_start(d), ob, "C")
        floor = lm.pixel_rel(r32["C"], r64["C"], keep)
        _report("cfit", cell, kind, "ridge %g" % ridge, int(ob.sum()), keep, acc, floor)
        _conditions(int(ob.sum()), keep, acc, floor)
    for sk, dl in ssr.KINDS:
        for color in (0, 1):
            r64, r32 = (lm.smooth_visit(cell, kind, SMOOTH_RIDGE, sk, dl, color, t)
                        for t in (np.float64, np.float32))
            own = r64["own"]
            keep, acc = lm.compared(r64, r32, lm.s_start(d), own)
            floor = lm.pixel_rel(r32["S"], r64["S"], keep)
            _report("smooth", cell, kind, "%s colour %d" % (sk, color), int(own.sum()), keep, acc,
                    floor)
            _conditions(int(own.sum()), keep, acc, floor)
            # the other colour does not move in the reference either
            assert np.array_equal(r64["S"][:, ~own], lm.s_start(d)[:, ~own])


@pytest.mark.parametrize("fitted", [0, 1])
@pytest.mark.parametrize("cell", CELL_IDS)
def test_check_flag_words_are_decided_away_from_the_guard(cell, fitted):
    """The flag words the GPU file compares exactly: at most 10 % of a cell's pixels (the
    allowance of the accept decisions) have I* / Ixx inside the guard's window, where fp32 may decide
    otherwise; the ladder's counts are the mask's."""
    ref = lm.check_stats(cell, fitted, CHECK_RIDGE, np.float64)
    ex = lm.check_excluded(ref)
    print("lm-host check %s fitted %d: not compared %d untestable %d" %
          (cell, fitted, int(ex.sum()), int((ref["flags"] & ckr.UNTESTABLE != 0).sum())))
    assert lm.check_excluded_ok(ex)
    assert ref["n"][0] == 0 and [int(ref["n"][n]) for n in lm.LADDER] == [1, 2, 3, 4, 5]
    assert ref["n"][lm.FULL_PIXEL] == lm.problem(cell)["K"]
    assert (ref["flags"] & (ckr.INVALID | ckr.SATURATED) == 0).all()


def test_the_16_bin_logit_finding():
    # the problem of the finding: sfit_ref.problem's recipe at R = 16, K = 70, 16 bins, sigma 0.3
    name = "list-matrix-finding"
    sr.CASES[name] = (16, 70, "bins16", None, 0.3, "logit", 22)
    try:
        d = sr.problem(name)
    finally:
        del sr.CASES[name]
        sr._PROB.pop(name, None)
    m = sr.model_of(d)
    R = d["R"]
    op = sr.observed_pixels(m["Wx"])
    truth = d["S"].reshape(R, lm.P).double().numpy()
    far, near = 0.8 * truth, lm.START["logit"] * truth
    # (i) the formula: h > 0 at every entry, and h = d g_x / d t by central differences
    T = m["C"].T @ far
    h = ir.curvature(T, m["Y"], m["b"], m["sigma"], 0.0, False, "logit", "observed")
    assert h.min() > 0
    e = ir.edges_of(m["b"], False)
    a = ir.link_scale(m["sigma"], "logit")
    Y = m["Y"].astype(np.int64)

    def score(t):
        Pr, P1, _ = ir.bin_terms(t, e[Y], e[Y + 1], a, "logit")
        return -P1 / Pr
    eps = 1e-5
    fd = (score(T + eps) - score(T - eps)) / (2 * eps)
    assert np.max(np.abs(fd - h)) <= 1e-6 * np.max(np.abs(h))
    # (ii) the blocks are positive definite, yet the undamped step from 0.8 S_true overshoots
    f0, g, Jb = sr.evaluate(far, ridge=1e-2, kind="observed", **m)
    assert min(np.linalg.eigvalsh(Jb[p]).min() for p in np.flatnonzero(op)) > 0
    step = np.abs(sr.chol_solve(Jb + 1e-2 * np.eye(R), (g + 1e-2 * far).T.copy(),
                                np.zeros(lm.P))[0]).max(axis=1)[op]
    assert np.median(step) > 1.0  # against |S| <= 1
    out = {}
    for where, S0 in (("far", far), ("near", near)):
        for kind in lm.KINDS:
            r = sr.fit(S0, ridge=1e-2, max_steps=1, mu0=0.0, kind=kind, **m)
            out[where, kind] = int(lm.moved(r, S0)[op].sum())
    print("lm-host finding: median |delta|_inf from 0.8 S_true", np.median(step), "accepted of",
          int(op.sum()), out)
    assert out["far", "observed"] == 0 and out["far", "expected"] > 0.9 * op.sum()
    assert out["near", "observed"] > 0.9 * op.sum() and out["near", "expected"] > 0.9 * op.sum()
    # (iii) with the damping the fit from the far start descends all the same
    r = sr.fit(far, ridge=1e-2, max_steps=30, mu0=1e-3, kind="observed", **m)
    assert (r["f"][op] < f0[op]).all()
