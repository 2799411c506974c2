"""CPU restatements for the clip-editing tests (TEST INFRASTRUCTURE): the sampler loop with a start step, an SDEdit start and a
masked pin of known latents, in fp32 torch on the oracle's schedule and denoiser; and the pixel-to-latent keep-mask reduction.

The loop follows VPSDEDPMPP2MSampler.__call__ (sampling.py:800-835) with its `sdedit` re-noising
`alpha_cumprod_sqrt[i] * known + randn * (1 - alpha_cumprod_sqrt[i]**2) ** 0.5` applied to the cells of a mask instead of the first
frames, drawn before the step's own draws; the steps themselves are oracle/sampler.py's."""
import torch

from oracle.sampler import DiffusionSamplerOracle, _ap


def mask_to_latent_ref(mask_px: torch.Tensor) -> torch.Tensor:
    """[F, Hp, Wp] (non-zero = keep) -> uint8 [(F + 3) // 4, Hp // 8, Wp // 8]: the minimum over each cell's block -- frame 0 alone,
    then groups of four frames; 8 x 8 pixels."""
    F, Hp, Wp = mask_px.shape
    assert F % 4 == 1 and Hp % 8 == 0 and Wp % 8 == 0
    m = (mask_px != 0).to(torch.uint8)
    t = torch.cat([m[:1], m[1:].reshape((F - 1) // 4, 4, Hp, Wp).amin(1)]) if F > 1 else m
    return t.reshape(t.shape[0], Hp // 8, 8, Wp // 8, 8).amin((2, 4))


def pin_ref(x, known, noise, mask, alpha, sigma):
    """latent_pin on the CPU: x, known, noise [..., T, C, H, W] fp32, mask [T, H, W] or None; alpha, sigma python floats or fp32
    scalars.  Three separately rounded fp32 operations where the mask is set, x elsewhere."""
    new = known if noise is None else alpha * known + sigma * noise
    if mask is None:
        return new.clone()
    return torch.where((mask != 0)[:, None].expand(x.shape[-4:]).expand(x.shape), new, x)


def edit_run_ref(cfg, network, x, randn_like, start=0, known=None, known_mask=None, known_noise=True):
    """DiffusionSampler.run(..., start, known, known_mask, known_noise) in fp32 on the CPU.  x: the initial noise [1, T, C, H, W];
    network as DiffusionSamplerOracle.run takes it.  Steps start .. num_steps - 1 run, the first of them first-order."""
    so = DiffusionSamplerOracle(cfg)
    a, ts = so.prepare()
    n = len(a) - 1
    cond = uc = torch.zeros(1, 2, 4)
    s_in = x.new_ones([x.shape[0]])
    x = x.clone()
    if known is not None and start > 0:
        x = a[start] * known + (1 - a[start] ** 2) ** 0.5 * x
    old = None
    for i in range(start, n):
        if known_mask is not None:
            rd = randn_like(x) if known_noise else None
            x = pin_ref(x, known, rd, known_mask, a[i], (1 - a[i] ** 2) ** 0.5)
        cur, nxt = s_in * a[i], s_in * a[i + 1]
        den, _ = so.denoise(network, x, cur, ts[-(i + 1)], cond, uc)
        if cfg.sampler == "ddim":
            a_t = ((1 - nxt ** 2) / (1 - cur ** 2)) ** 0.5
            x = _ap(a_t, x) * x + _ap(nxt - cur * a_t, x) * den
            continue
        if i == n - 1:
            x = den
            continue
        ac, acn = cur ** 2, nxt ** 2
        lamb = ((ac / (1 - ac)) ** 0.5).log()
        h = ((acn / (1 - acn)) ** 0.5).log() - lamb
        m1 = ((1 - nxt ** 2) / (1 - cur ** 2)) ** 0.5 * (-h).exp()
        m2 = (-2 * h).expm1() * nxt
        mn = (1 - nxt ** 2) ** 0.5 * (1 - (-2 * h).exp()) ** 0.5
        n1 = randn_like(x)
        if old is None:
            x, old = _ap(m1, x) * x - _ap(m2, x) * den + _ap(mn, x) * n1, den
            continue
        acp = (s_in * a[i - 1]) ** 2
        r = (lamb - ((acp / (1 - acp)) ** 0.5).log()) / h
        den_d = _ap(1 + 1 / (2 * r), x) * den - _ap(1 / (2 * r), x) * old
        x = _ap(m1, x) * x - _ap(m2, x) * den_d + _ap(mn, x) * randn_like(x)       # the first draw is discarded, as in the reference
        old = den
    if known_mask is not None:
        x = pin_ref(x, known, None, known_mask, 1.0, 0.0)
    return x
