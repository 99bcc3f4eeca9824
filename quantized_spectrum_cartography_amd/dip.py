"""Deep-image-prior solver — defines the reference's empty qmc/dip.py entry point.

The reference ships qmc/dip.py as a 0-byte file and its notebook is missing
(.MISSING_LARGE_BLOBS:4); the only DIP artefact is the decoder architecture
deep_prior/networks/dip.py:20-89.  This module defines the solver the way the reference's
GAN solver works (qmc/qmc.ipynb :559-634): alternating fused HIP C-steps with S-steps that
back-propagate the fused HIP dS through a decoder S = D_theta(Z).  Choices (documented in
DESIGN.md): the S-step optimises the decoder weights theta with the input Z fixed (classic DIP;
`optimize="z"` optimises Z only, as the GAN path does); BatchNorm runs in eval mode so the R
emitters are decoded independently and deterministically.
"""
import torch

from .nets import DecoderDip, SizedDecoderDip
from .obs import Observations
from .qmc import GeneratorSolver, drive_generator
from .utils import LOG_OFFSET_7_ADJUSTED as LOG_OFFSET


def make_decoder(I, J, zdim=256, seed=0, ndf=16):
    """A DIP decoder for I x J maps: the reference's DecoderDip at 51 x 51 (zdim 256, ndf 16),
    SizedDecoderDip otherwise (`ndf` sets its widths; 16 is the reference's)."""
    if I != J:
        raise ValueError("the DIP decoder produces square maps")
    g = torch.Generator().manual_seed(seed)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(int(torch.randint(0, 2 ** 31 - 1, (1,), generator=g)))
        net = (DecoderDip() if (I == 51 and zdim == 256 and ndf == 16)
               else SizedDecoderDip(I, zdim, ndf=ndf))
    return net


@torch.no_grad()
def calibrate_bn(decoder, Z):
    """Data-dependent initialisation of the decoder's BatchNorm layers: their running statistics
    set to the batch statistics of one forward pass at Z (train mode, momentum 1), then eval
    mode.  A freshly initialised decoder run in eval mode (unit running variance) lets the
    activations of its ~16 conv layers drift far from unit scale and the output sigmoid
    saturate, where a pre-fit to a warm start no longer moves it; after calibration every BN
    layer normalises the activations Z actually produces, and the R emitters still decode
    independently (eval mode)."""
    bns = [m for m in decoder.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    saved = [(m.momentum, m.training) for m in bns]
    decoder.train()
    for m in bns:
        m.reset_running_stats()
        m.momentum = 1.0
    decoder(Z)
    for m, (mom, _) in zip(bns, saved):
        m.momentum = mom
    decoder.eval()
    return decoder


def prefit(decoder, Z, S_target, steps=1000, lr=1e-2, peak=0.9):
    """Fit the decoder's output to a warm-start S (e.g. warm.warm_start), fields scaled to
    `peak` at their maximum (the sigmoid output's range).  Returns the scale s: the decoder then
    represents S_target / s, so C_init * s keeps T_hat = S C."""
    R = S_target.shape[0]
    I, J = S_target.shape[-2], S_target.shape[-1]
    S_target = S_target.detach().to(Z.device, torch.float32).reshape(R, 1, I, J)
    s = float(S_target.max()) / peak if float(S_target.max()) > 0 else 1.0
    target = (S_target / s).clamp(1e-4, peak)
    opt = torch.optim.Adam(decoder.parameters(), lr=lr)
    for _ in range(int(steps)):
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(decoder(Z).reshape(R, 1, I, J), target)
        loss.backward()
        opt.step()
    return s


def solve(Y, Wx, bin_boundaries, noise_std, R, offset=None, log_model=True, decoder=None,
          Z_init=None, C_init=None, lambda_c=100.0, lambda_s=100.0, lr_c=5e-3, lr_s=1e-2,
          max_iter=500, optimize="weights", T_true=None, nmse_every=0, obs=None, tile=None,
          seed=0, callback=None, S_init=None, prefit_steps=1000, prefit_lr=1e-2, ndf=16,
          warm="residual", residual_scale=None, lr_c_rel=1e-2, calibrate=True, use_graph=True,
          build_only=False, hist_cap=None, loss="probit"):
    """DIP-regularised alternating probit MLE (config 5: log model + DIP prior on S).

    loss: "probit" (default), "logit" (the logistic link, noise_std its scale s) or "squared",
    as qmc.solve; ignored when a packed `obs` is given (its model decides).

    `offset` defaults to the reference log model's LOG_OFFSET_7_ADJUSTED
    (qmc/quantization_model_log.py:7, 9): with the zero C_init the first C-pass sees
    T_hat = 0, and log(0 + offset) must stay finite.

    Warm start (the notebook's optional warm start, qmc/qmc.ipynb :513-516), S_init (R,1,I,J)
    and C_init (e.g. warm.warm_start):
      warm="residual" (default): S = max(S_init + a (D(Z) - D(Z_0)), 0) with D(Z_0) the
        decoder's output at the start (a constant): the solve starts exactly at the warm
        start's map and the decoder parameterises the correction, a DIP prior on the update
        (a = residual_scale, default the warm-start fields' mean absolute value);
      warm="relative": S = S_init exp(a (D(Z) - D(Z_0))) (a default 1): the correction is
        relative, so S stays > 0 wherever S_init is and small values keep their scale (the log
        model's domain);
      warm="prefit": the decoder itself is pre-fitted to S_init (`prefit_steps` Adam steps at
        `prefit_lr`) and C_init rescaled by the pre-fit's field scale (a 256 x 256 decoder of
        the reference's widths cannot reproduce the fields' peaks: profiles/r04/c5_explore*).
    calibrate=True (default since round 4): a decoder built here is BN-calibrated at Z_init
    (calibrate_bn) -- a data-dependent initialisation the reference does not have (its DIP
    notebook is not shipped), so the cold-start numbers differ from an uncalibrated decoder's
    (parity unpinned); calibrate=False keeps the fresh BatchNorm statistics.

    lr_c="auto": the C-step's Adam step sized to the data instead of the notebook's absolute 5e-3
    (qmc/qmc.ipynb :549), which assumes maps of unit scale: lr_c = lr_c_rel x c_target with
    c_target = mean(T_hat) / (R mean(S_start)), T_hat the de-quantized map (warm.dequantize) and
    S_start the S the solve starts from -- so from the notebook's zero C the C-step reaches the
    data's scale in ~1/lr_c_rel steps instead of overshooting it by orders of magnitude (a
    generated C5 map has T ~ 1e-5: at 5e-3 the cold start oscillates to map NMSE ~4, profiles/r04/
    quality.json).  The value used is returned as result.lr_c.

    use_graph=True (default): after one eager iteration the iterations run as captured hipGraph
    chunks (qmc.GeneratorSolver: decoder forward / backward, its optimizer step and the fused HIP
    passes, no host synchronisation per iteration); result.graph_error says why not if a capture
    failed.  build_only=True returns the qmc.GeneratorSolver without running it (bench.py's
    --config c5dip times its run(); hist_cap bounds its cost history, default max_iter)."""
    if log_model:
        offset = LOG_OFFSET if offset is None else float(offset)
        if not offset > 0.0:
            raise ValueError("the log model needs offset > 0 (log(T_hat + offset) at T_hat = 0)")
    K = Y.shape[0]
    I, J = Y.shape[-2], Y.shape[-1]
    if obs is None:
        obs = Observations(Y, Wx, bin_boundaries, noise_std, offset=offset if log_model else 0.0,
                           log_model=log_model, tile=tile, R_hint=R, loss=loss)
    dev = obs.device
    fresh = decoder is None
    if fresh:
        decoder = make_decoder(I, J, seed=seed, ndf=ndf)
    decoder = decoder.to(dev).eval()
    if Z_init is None:
        g = torch.Generator().manual_seed(seed + 1)
        Z_init = torch.randn((R, 256), generator=g)
    if C_init is None:
        C_init = torch.zeros(R, K)
    if fresh and calibrate:
        calibrate_bn(decoder, Z_init.detach().to(dev, torch.float32))
    net = decoder
    if S_init is not None and warm == "prefit":
        if not fresh:
            raise ValueError("warm='prefit' pre-fits the decoder built here; pass decoder=None")
        scale = prefit(decoder, Z_init.detach().to(dev, torch.float32), S_init,
                       steps=prefit_steps, lr=prefit_lr)
        C_init = C_init.detach().to(torch.float32) * scale
        decoder.eval()
    elif S_init is not None:
        if warm not in ("residual", "relative"):
            raise ValueError("warm must be 'residual', 'relative' or 'prefit'")
        base = S_init.detach().to(dev, torch.float32).reshape(R, 1, I, J)
        if warm == "residual":
            a = float(base.abs().mean()) if residual_scale is None else float(residual_scale)
        else:
            a = 1.0 if residual_scale is None else float(residual_scale)
        with torch.no_grad():
            d0 = decoder(Z_init.detach().to(dev, torch.float32)).reshape(R, 1, I, J).clone()
        net = _Residual(decoder, base, d0, a, relative=warm == "relative")
    for p in decoder.parameters():
        p.requires_grad_(optimize in ("weights", "both"))
    params = []
    if optimize in ("weights", "both"):
        params += list(decoder.parameters())
    Zp = Z_init.detach().to(dev, torch.float32).clone()
    if isinstance(lr_c, str):
        if lr_c != "auto":
            raise ValueError("lr_c must be a number or 'auto'")
        with torch.no_grad():
            s_mean = float(net(Zp).abs().mean())
        lr_c = float(lr_c_rel) * _c_target(Y, Wx, bin_boundaries, noise_std, R, s_mean,
                                            offset if log_model else 0.0, log_model)
    sol = GeneratorSolver(obs, net, Zp, C_init, R, lambda_c, lambda_s, lr_c, lr_s,
                          (0.9, 0.999), 1e-8, True, params=params,
                          optimize_z=optimize in ("z", "both"), hist_cap=hist_cap or max_iter)
    sol.decoder = decoder
    sol.lr_c = float(lr_c)
    if build_only:
        return sol
    res = drive_generator(sol, max_iter, False, (0, 0), T_true, nmse_every, callback, use_graph)
    res.decoder = decoder
    res.lr_c = float(lr_c)
    return res


def _c_target(Y, Wx, bin_boundaries, noise_std, R, s_mean, offset, log_model):
    """mean(T_hat) / (R s_mean): the magnitude of C at which T_hat = S C has the de-quantized
    data's scale (dip.solve lr_c="auto")."""
    from .warm import dequantize
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    xh = dequantize(Y.to(dev), Wx.to(dev) if Wx is not None else None, bin_boundaries,
                    noise_std)
    t = (torch.exp(xh) - float(offset)).clamp_min(0.0) if log_model else xh.clamp_min(0.0)
    return float(t.mean()) / (R * max(s_mean, 1e-30))


class _Residual(torch.nn.Module):
    """S = max(base + a (D(Z) - d0), 0) (dip.solve warm="residual") or base exp(a (D(Z) - d0))
    (warm="relative"): the warm-start map with a decoder-parameterised correction; S >= 0 as the
    reference's sigmoid-output S."""

    def __init__(self, decoder, base, d0, a, relative=False):
        super().__init__()
        self.decoder = decoder
        self.register_buffer("base", base)
        self.register_buffer("d0", d0)
        self.a = a
        self.relative = relative

    def forward(self, z):
        d = self.decoder(z).reshape(self.base.shape)
        if self.relative:
            return self.base * torch.exp(self.a * (d - self.d0))
        return torch.clamp_min(self.base + self.a * (d - self.d0), 0.0)
