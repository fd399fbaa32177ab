"""Shared inputs and the fp64 reference of the fused optimizer step (tests/test_optim_host.py, tests/test_optim_gpu.py).

The reference is the formula of include/gvf_optim.h in torch double.  The conformance bars are STAGED: every output of the kernel is
compared with the fp64 formula evaluated on the kernel's own fp32 inputs to that stage (its gc, its m' and v', its p'), so each bar
counts only the roundings of that stage.  E = 2^-24 is the unit round-off of fp32."""
import torch

E = 2.0 ** -24
LRS, WDS = (1e-4, 1e-5), (0.01, 0.0)
BETAS, EPS = (0.9, 0.999), 1e-8
EMA_RATES = (0.9999, 0.999)
GUARD = 12345.0


def ragged_sizes(C, big=True):
    """The ragged tensor set of the issue for chunk length C (the misaligned view of 1001 elements is appended by make_params)."""
    sizes = [1, 3, 4, 5, 16, 63, 64, 65, 255, 1023, 1024, 1025, C - 1, C, C + 1, 2 * C + 7, 0]
    if big:
        sizes.append(3 * 2 ** 20 + 5)
    return sizes


def make_params(device, C, seed=0, big=True):
    """Parameters N(0, 0.05^2) over ragged_sizes plus one contiguous parameter that is a view at a 4-byte offset (scalar path)."""
    g = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter((0.05 * torch.randn(n, generator=g)).to(device)) for n in ragged_sizes(C, big)]
    base = torch.empty(1002, device=device)
    base.copy_(0.05 * torch.randn(1002, generator=g))
    base[0] = GUARD
    params.append(torch.nn.Parameter(base[1:]))
    params[-1].guard_base = base                       # base[0] sits 4 bytes in front of the parameter
    assert params[-1].data_ptr() % 16 == 4 and params[-1].is_contiguous()
    return params


def groups_of(params):
    """Two groups: even-numbered tensors at lr 1e-4 / weight decay 0.01, odd-numbered ones at lr 1e-5 / 0."""
    return [{"params": params[0::2], "lr": LRS[0], "weight_decay": WDS[0]}, {"params": params[1::2], "lr": LRS[1], "weight_decay": WDS[1]}]


def group_index(params):
    return [i % 2 for i in range(len(params))]


def make_grads(params, seed=1, sigma=None):
    """N(0, 1) times 10^U(-8, 0) per element (sigma=None), or N(0, sigma^2)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for p in params:
        x = torch.randn(p.numel(), generator=g)
        x = x * (10.0 ** (-8.0 * torch.rand(p.numel(), generator=g))) if sigma is None else x * sigma
        out.append(x.to(p.device).view(p.shape))
    return out


def make_moments(params, seed=2):
    """Non-zero Adam moments: m ~ N(0, 1e-2^2), v = (N(0, 1e-2^2))^2 + 1e-12."""
    g = torch.Generator().manual_seed(seed)
    ms = [(1e-2 * torch.randn(p.numel(), generator=g)).to(p.device).view(p.shape) for p in params]
    vs = [((1e-2 * torch.randn(p.numel(), generator=g)) ** 2 + 1e-12).to(p.device).view(p.shape) for p in params]
    return ms, vs


def set_state(opt, params, step, ms, vs):
    """Moments and step count through the public path: a state dict in torch.optim.AdamW's layout."""
    sd = opt.state_dict()
    index = {id(p): i for i, p in enumerate(q for group in opt.param_groups for q in group["params"])}
    sd["state"] = {index[id(p)]: {"step": torch.tensor(float(step)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
                   for p, m, v in zip(params, ms, vs)}
    opt.load_state_dict(sd)


def ema_views(opt, params, k):
    """The k-th EMA copies in the order of `params` (opt.ema_params follows the parameter groups)."""
    order = {id(q): j for j, q in enumerate(q for group in opt.param_groups for q in group["params"] if q.requires_grad)}
    e = opt.ema_params(k)
    return [e[order[id(p)]] for p in params]


def snapshot(opt, params):
    """Bit-exact copies of everything a step writes."""
    return {"p": [p.detach().clone() for p in params], "m": [opt.state[p]["exp_avg"].clone() for p in params],
            "v": [opt.state[p]["exp_avg_sq"].clone() for p in params],
            "ema": [[e.clone() for e in ema_views(opt, params, k)] for k in range(len(opt.ema_rates))],
            "grad_norm": opt.grad_norm.clone(), "found_inf": opt.found_inf.clone(), "clip_coef": opt.clip_coef.clone(),
            "step": opt.step_count.clone()}


def snapshots_equal(a, b):
    for key in ("p", "m", "v"):
        if not all(torch.equal(x, y) for x, y in zip(a[key], b[key])):
            return False
    for ea, eb in zip(a["ema"], b["ema"]):
        if not all(torch.equal(x, y) for x, y in zip(ea, eb)):
            return False
    return all(torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                           b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k])
               for k in ("grad_norm", "found_inf", "clip_coef", "step"))


def norm_f64(grads, inv_scale=1.0):
    """sqrt(sum gu^2) in double over gu = fp32(g * inv_scale)."""
    inv = torch.tensor(inv_scale, dtype=torch.float32)
    s = 0.0
    for g in grads:
        gu = (g.float() * inv.to(g.device)).double()
        s += float((gu * gu).sum())
    return s ** 0.5


def torch_clip_coef(norm32_cpu, max_norm):
    """torch.nn.utils.clip_grad_norm_'s coefficient from the fp32 total norm (a CPU tensor)."""
    return torch.clamp(max_norm / (norm32_cpu + 1e-6), max=1.0)


def _worst(err, bar):
    """max over elements of err / bar (0 where both vanish)."""
    if err.numel() == 0:
        return 0.0
    r = torch.where(bar > 0, err / bar, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


def staged_errors(before, after, grads, groups, step, lrs=LRS, wds=WDS, inv_scale=1.0, skipped=False):
    """Worst element-wise error of every output in units of E x (the magnitudes of its bar): {"m": .., "v": .., "p": .., "ema": ..}.
    `step` is the step count the update used (the count after the increment).  The bars of the issue are m 4, v 4, p 8, ema 4.
    skipped: the step found a non-finite norm; only the EMAs are compared (toward the unchanged p)."""
    b1, b2 = BETAS
    clip = after["clip_coef"]
    out = {"m": 0.0, "v": 0.0, "p": 0.0, "ema": 0.0}
    for i, g in enumerate(grads):
        p0, m0, v0 = before["p"][i].double(), before["m"][i].double(), before["v"][i].double()
        p1, m1, v1 = after["p"][i].double(), after["m"][i].double(), after["v"][i].double()
        if not skipped:
            inv = torch.tensor(inv_scale, dtype=torch.float32, device=g.device)
            gc = ((g * inv) * clip).double()                     # the kernel's own fp32 gc
            lr, wd = lrs[groups[i]], wds[groups[i]]
            a, b = b1 * m0, (1.0 - b1) * gc
            out["m"] = max(out["m"], _worst((m1 - (a + b)).abs(), E * (a.abs() + b.abs())))
            a, b = b2 * v0, (1.0 - b2) * gc * gc
            out["v"] = max(out["v"], _worst((v1 - (a + b)).abs(), E * (a.abs() + b.abs())))
            bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
            u = (lr / bc1) * m1 / (v1.sqrt() / bc2 ** 0.5 + EPS)  # from the kernel's m', v'
            a = p0 * (1.0 - lr * wd)
            out["p"] = max(out["p"], _worst((p1 - (a - u)).abs(), E * (a.abs() + u.abs())))
        for k, r in enumerate(EMA_RATES[:len(after["ema"])]):
            e0, e1 = before["ema"][k][i].double(), after["ema"][k][i].double()
            a, b = r * e0, (1.0 - r) * p1                        # toward the kernel's p'
            out["ema"] = max(out["ema"], _worst((e1 - (a + b)).abs(), E * (a.abs() + b.abs())))
    return out


BARS = {"m": 4.0, "v": 4.0, "p": 8.0, "ema": 4.0}


def assert_within_bars(errs, what=""):
    print(f"{what} staged errors in units of E x magnitude: " + ", ".join(f"{k} {v:.3f} (bar {BARS[k]})" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= BARS[k], f"{what}: {k} is {v:.3f} E x magnitude, bar {BARS[k]}"
