"""CPU: the split of the post-solve estimators into fits.py -- qmc re-exports the very objects,
fits does not import qmc, the one stepping loop's read-back cadence, the one table of
solve()'s post-solve option rules, and the order of the post-solve stage.  No device."""
import os
import subprocess
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every moved name that tests, tools, bench.py or the package reach as qmc.NAME
REEXPORTS = ("INFO_KINDS", "confidence", "default_confidence_ridge", "fit_S", "fit_C", "fit_noise",
             "fit_S_smooth", "model_nll", "calibrate", "FitSResult", "FitCResult",
             "check_fit_noise", "check_polish_c", "check_confidence", "shifted_boundaries",
             "_fit_s_pos", "_fit_c_pos", "_fit_noise_pos", "_sfit_smooth_bufs",
             "_sfit_smooth_visit", "_fit_s_smooth_pos")


def test_qmc_reexports_the_objects_of_fits():
    from quantized_spectrum_cartography_amd import fits, qmc
    for n in REEXPORTS:
        assert getattr(qmc, n) is getattr(fits, n), n


def test_fits_does_not_import_qmc():
    code = ("import sys\n"
            "import quantized_spectrum_cartography_amd.fits\n"
            "assert 'quantized_spectrum_cartography_amd.qmc' not in sys.modules\n")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)


def _recorders(active_values=()):
    calls = []
    values = list(active_values)

    def step():
        calls.append("step")

    def active():
        calls.append("active")
        return values.pop(0) if values else 1
    return calls, step, active


def test_iterate_reads_back_every_sync_every_steps_and_stops_at_zero():
    from quantized_spectrum_cartography_amd.fits import _iterate
    calls, step, active = _recorders()
    assert _iterate(step, 7, 0, active) == 7
    assert calls == ["step"] * 7  # sync_every = 0: no read-back (capturable)
    calls, step, active = _recorders([1, 0])
    assert _iterate(step, 10, 4, active) == 8
    assert calls == ["step"] * 4 + ["active"] + ["step"] * 4 + ["active"]
    calls, step, active = _recorders()
    assert _iterate(step, 10, 4, active) == 10
    assert calls.count("step") == 10 and calls.count("active") == 2
    calls, step, active = _recorders()
    assert _iterate(step, 0, 4, active) == 0 and calls == []


OPTIONS = ("polish_s", "polish_c", "polish_smooth", "calibrate", "confidence")


def _on(option):
    """The keywords that switch one option on, with the smooth it needs."""
    kw = {option: "expected" if option == "confidence" else 3}
    return kw, (0.1 if option == "polish_smooth" else 0.0)


@pytest.mark.parametrize("option", OPTIONS)
def test_post_solve_options_share_one_table_of_rules(option):
    from quantized_spectrum_cartography_amd.fits import check_post_solve
    kw, smooth = _on(option)
    with pytest.raises(ValueError, match="generator") as e:
        check_post_solve(object(), "probit", smooth, **kw)
    assert option in str(e.value)
    with pytest.raises(ValueError, match="squared"):
        check_post_solve(None, "squared", smooth, **kw)
    post = check_post_solve(None, "logit", smooth, **kw)
    assert getattr(post, option) == kw[option]
    assert all(getattr(post, o) == (None if o == "confidence" else 0)
               for o in OPTIONS if o != option)
    if option != "confidence":  # (confidence is a kind, not a count)
        with pytest.raises(ValueError, match=option):
            check_post_solve(None, "probit", smooth, **{option: -1})
        # off: neither a generator nor the squared loss is refused
        assert getattr(check_post_solve(object(), "squared", smooth, **{option: 0}), option) == 0


def test_post_solve_keeps_the_rules_of_each_option():
    from quantized_spectrum_cartography_amd.fits import check_post_solve
    with pytest.raises(ValueError, match="couples pixels"):
        check_post_solve(None, "probit", 0.1, polish_s=3)
    with pytest.raises(ValueError, match="smooth > 0"):
        check_post_solve(None, "probit", 0.0, polish_smooth=3)
    assert check_post_solve(None, "probit", 0.1, polish_c=3).polish_c == 3
    with pytest.raises(ValueError, match="kind"):
        check_post_solve(None, "probit", 0.0, confidence="laplace")
    with pytest.raises(ValueError, match="ridge"):
        check_post_solve(None, "probit", 0.0, confidence="expected", confidence_ridge=-1.0)
    post = check_post_solve(object(), "squared", 0.0)
    assert (post.polish_s, post.polish_c, post.polish_smooth, post.calibrate,
            post.confidence) == (0, 0, 0, 0, None)


def _stub_steps(monkeypatch):
    """Replace the five step functions of fits by recorders; -> (calls, the calibrated obs)."""
    from quantized_spectrum_cartography_amd import fits
    calls = []
    obs_cal = object()
    S, C = torch.ones(2, 1, 3, 5), torch.ones(2, 4)

    def rec(name, **result):
        def f(obs, *a, **kw):
            calls.append((name, obs))
            return types.SimpleNamespace(**result)
        return f
    monkeypatch.setattr(fits, "fit_C", rec("polish_c", C=2 * C))
    monkeypatch.setattr(fits, "fit_S", rec("polish_s", S=2 * S))
    monkeypatch.setattr(fits, "fit_S_smooth", rec("polish_smooth", S=3 * S))
    monkeypatch.setattr(fits, "calibrate", rec("calibrate", S=4 * S, C=4 * C, obs=obs_cal))
    monkeypatch.setattr(fits, "confidence", rec("confidence", std_S=5 * S, unidentified=7))
    return calls, obs_cal


def _result():
    from quantized_spectrum_cartography_amd import qmc
    return qmc.SolveResult(S=torch.ones(2, 1, 3, 5), C=torch.ones(2, 4), costs_c=[], costs_s=[])


def test_post_solve_runs_the_steps_in_order_and_hands_the_calibrated_obs_on(monkeypatch):
    from quantized_spectrum_cartography_amd import fits
    calls, obs_cal = _stub_steps(monkeypatch)
    obs = object()
    post = fits.PostSolve(polish_c=1, polish_s=2, polish_smooth=3, calibrate=1,
                          confidence="expected")
    res = fits.post_solve(_result(), obs, post, 100.0, 100.0, None, 0.1, "quad", None)
    assert [c[0] for c in calls] == ["polish_c", "polish_s", "polish_smooth", "calibrate",
                                     "confidence"]
    assert all(o is obs for _, o in calls[:4]) and calls[4][1] is obs_cal
    # each step's result lands in res, and the fit's own copy of S / C is dropped
    assert float(res.S[0, 0, 0, 0]) == 4.0 and float(res.C[0, 0]) == 4.0
    assert res.polish_c.C is None and res.polish.S is None and res.polish_smooth.S is None
    assert res.calibration.S is None and res.calibration.C is None
    assert res.calibration.obs is obs_cal
    assert float(res.std_S[0, 0, 0, 0]) == 5.0 and res.unidentified == 7


def test_post_solve_with_every_option_off_calls_nothing(monkeypatch):
    from quantized_spectrum_cartography_amd import fits
    calls, _ = _stub_steps(monkeypatch)
    r = _result()
    assert fits.post_solve(r, object(), fits.PostSolve(), 100.0, 100.0, None, 0.0, "quad",
                           None) is r
    assert calls == []
    assert r.polish is None and r.polish_c is None and r.polish_smooth is None
    assert r.calibration is None and r.std_S is None
