"""Generate the logistic (ordered-logit) golden vectors from the REFERENCE implementation.

Companion of tools/make_golden.py, run only where the read-only reference tree is available
(same location).  It imports the reference's own F_sigmoid, get_tensor and quantize at run time
(qmc/quantization_model.py, qmc/quantization_model_log.py; nothing is copied) and re-enacts the
C-step / S-step of qmc/qmc.ipynb cell 1 (:559-634, S the free Adam variable, as make_golden.py)
with the likelihood formed from the reference's logistic CDF,
    P = F_sigmoid((U - X)/s) - F_sigmoid((W - X)/s)      (autograd guarded at the clamp, see guarded()),
U, W the upper / lower bin edges with prob_probit's edge handling (qmc/quantization_model.py
:31-36: linear b[0] = -1e5, b[-1] = 1e5; quantization_model_log.py:32-36: raw edges).

Writes tests/golden/pass_logit_small.npz (linear one-bit, 3 x 16 x 16 x 12) and
tests/golden/solve_logit_32.npz (log model, 4 bins, 3 x 32 x 32 x 16, 10 iterations): the inputs,
NLL / cost / dS / dC from autograd at the start, S and C after iterations 1 and n, and the cost
histories.

Every observed entry of the inputs must have reference-fp32 P >= 0.05 (asserted): the
reference's 1/(1+exp(-y)) loses its relative precision where 1 - F cancels, and the goldens
should pin the model, not that cancellation.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_logit.py
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")

sys.dont_write_bytecode = True
sys.path += [os.path.join(REF, "qmc"), os.path.join(REF, "deep_prior")]
import quantization_model as qm  # noqa: E402
import quantization_model_log as qml  # noqa: E402

torch.set_num_threads(1)  # deterministic CPU reductions for the fixtures
P_MIN = 0.05


def f32(t):
    return t.detach().cpu().numpy().astype(np.float32)


def guarded(z):
    """The reference's F_sigmoid(z), values unchanged.  Where exp(-z) overflows (the linear
    model's -1e5 clamp edge: F == 0 exactly) the reference's autograd forms 0 * inf = nan; that
    term is a constant, so it is evaluated detached and the differentiated call gets z = 0 there.
    """
    sat = torch.isinf(torch.exp(-z.detach()))
    return torch.where(sat, qm.F_sigmoid(z.detach()),
                       qm.F_sigmoid(torch.where(sat, torch.zeros_like(z), z)))


def prob_logit(Y, X_hat, b, s, log_model):
    b = b.clone()
    if not log_model:
        b[0] = -100000
        b[-1] = 100000
    W = b[Y]
    U = b[Y + 1]
    return guarded((U - X_hat) / s) - guarded((W - X_hat) / s)


def nll_cost(S, C, d, lam_c, lam_s):
    T_hat = qm.get_tensor(S, C).unsqueeze(1)
    if d["log_model"]:
        T_hat = torch.log(T_hat + d["offset"])
    P = prob_logit(d["Y"], T_hat, d["b"], d["s"], d["log_model"])
    nll = -torch.sum(d["Wx"] * torch.log(P))
    return nll, nll + lam_c * torch.norm(C, "fro") + lam_s * torch.norm(S, "fro"), P


def synth_onebit(seed, R, I, J, K, f=0.3):
    """make_golden.synth_onebit's recipe: threshold at the median, s = (max - min) / 4."""
    torch.manual_seed(seed)
    S_true = torch.rand(R, 1, I, J)
    C_true = torch.rand(R, K)
    T_true = qm.get_tensor(S_true, C_true)
    thr = float(T_true.median())
    tmax, tmin = float(T_true.max()), float(T_true.min())
    s = float(np.float32((tmax - tmin) / 4))  # stored as fp32: keep it representable
    b = torch.tensor([0.0, thr, tmax])
    Y = qm.quantize(T_true, s, b).unsqueeze(1)
    Wx = torch.bernoulli(torch.full((K, 1, I, J), f))
    S0 = 0.5 * torch.rand(R, 1, I, J)
    C0 = 0.5 * torch.rand(R, K)
    return dict(T_true=T_true, b=b, s=s, Y=Y, Wx=Wx, S0=S0, C0=C0, offset=0.0, log_model=False)


def synth_log(seed, R, I, J, K, f=0.3):
    """Log model, 4 bins, raw edges c + s * (-8, -1, 0, 1, 8) around the median c of
    log(T_true + offset), with s = max |x - c| / 1.5 over the true map and the starting point:
    an entry at most 1.5 s from c sees every bin with P >= F(-2.5) = 0.076 >= P_MIN."""
    torch.manual_seed(seed)
    S_true = 0.25 + 0.5 * torch.rand(R, 1, I, J)
    C_true = torch.rand(R, K)
    T_true = qm.get_tensor(S_true, C_true)
    S0 = 0.25 + 0.5 * torch.rand(R, 1, I, J)
    C0 = 0.5 * torch.rand(R, K)
    off = 1e-3
    x = torch.log(T_true + off)
    x0 = torch.log(qm.get_tensor(S0, C0) + off)
    c = float(x.median())
    s = float(np.float32(max(float((x - c).abs().max()), float((x0 - c).abs().max())) / 1.5))
    b = torch.tensor([c - 8 * s, c - s, c, c + s, c + 8 * s])
    Y = qml.quantize(T_true, s, b, offset=off).unsqueeze(1)
    Wx = torch.bernoulli(torch.full((K, 1, I, J), f))
    return dict(T_true=T_true, b=b, s=s, Y=Y, Wx=Wx, S0=S0, C0=C0, offset=off, log_model=True)


def gen(name, d, n_iter, lam_c=100.0, lam_s=100.0, lr_c=5e-3, lr_s=1e-2):
    S = d["S0"].clone().requires_grad_(True)
    C = d["C0"].clone().requires_grad_(True)
    nll, cost, P = nll_cost(S, C, d, lam_c, lam_s)
    pmin = float(P.detach()[d["Wx"] != 0].min())
    assert pmin >= P_MIN, "%s: an observed entry has reference P = %g < %g" % (name, pmin, P_MIN)
    cost.backward()
    out = dict(S0=f32(d["S0"]), C0=f32(d["C0"]), Y=d["Y"].numpy().astype(np.uint8),
               Wx=f32(d["Wx"]).astype(np.uint8), b=f32(d["b"]), sigma=np.float32(d["s"]),
               offset=np.float64(d["offset"]), log_model=np.int32(d["log_model"]),
               lam_c=np.float32(lam_c), lam_s=np.float32(lam_s), lr_c=np.float32(lr_c),
               lr_s=np.float32(lr_s), n_iter=np.int32(n_iter), p_min=np.float32(pmin),
               nll=np.float64(nll.item()), cost=np.float64(cost.item()), dS=f32(S.grad),
               dC=f32(C.grad))
    # the alternating loop (make_golden.gen_solve with the logistic likelihood)
    S = d["S0"].clone().requires_grad_(True)
    C = d["C0"].clone().requires_grad_(True)
    optC = torch.optim.Adam([C], lr=lr_c)
    optS = torch.optim.Adam([S], lr=lr_s)
    costs_c, costs_s = [], []
    for i in range(n_iter):
        Sc = S.detach().clone()
        optC.zero_grad()
        _, cost, _ = nll_cost(Sc, C, d, lam_c, lam_s)
        cost.backward()
        optC.step()
        with torch.no_grad():
            C[C < 0] = 0
        costs_c.append(cost.item())
        optS.zero_grad()
        _, cost, _ = nll_cost(S, C, d, lam_c, lam_s)
        cost.backward()
        optS.step()
        costs_s.append(cost.item())
        if i + 1 in (1, n_iter):
            out["S_it%d" % (i + 1)] = f32(S)
            out["C_it%d" % (i + 1)] = f32(C)
    out["costs_c"], out["costs_s"] = np.array(costs_c), np.array(costs_s)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, torch_version=np.array(torch.__version__), **out)
    print("wrote", path, os.path.getsize(path), "bytes; min observed P", pmin)


def main():
    os.makedirs(OUT, exist_ok=True)
    gen("pass_logit_small", synth_onebit(20270, 3, 16, 16, 12), n_iter=5)
    gen("solve_logit_32", synth_log(20271, 3, 32, 32, 16), n_iter=10)


if __name__ == "__main__":
    main()
