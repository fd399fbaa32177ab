"""fp64 reference of the LPIPS (VGG16) operator (include/gvf_lpips.h, gvfdiffusion_amd/ops/lpips.py), in torch on the CPU: the whole
composition (trunk, taps, loss; pinned to the reference's own code by tests/golden/lpips_golden.npz) and per-stage references with
their error bounds.  Nothing here depends on downloaded VGG weights: seeded_weights() makes a full state dict, with the reference's
key names, from a counter-based integer hash in numpy uint64 arithmetic (no library RNG stream, so the bits are the same everywhere).

Bounds.  The convolution is a GEMM with K = 9 Cin: gvf_conv3x3 takes exactly ceil(9 Cin / 32) MFMA k-steps (Cin / 32 chunks times nine
taps; the first layer's K = 27 is one zero-padded step), which is what gemm_ref.accumulation_error(9 Cin, ...) counts; an addend is one
more fp32 add.  ReLU is monotone and 1-Lipschitz, so it carries the bound unchanged, and gemm_ref._round_bound takes it to the 16-bit
output.  A masked element must be exactly zero.  The first layer's input gradient is a sequential fp32 fma chain of 9 * 64 terms and
one division."""
import numpy as np
import torch
import torch.nn.functional as F

from gemm_ref import U32, _round_bound, accumulation_error

VGG_CONVS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256), (17, 256, 512),
             (19, 512, 512), (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512))
POOL_AFTER = (1, 3, 6, 9)
TAPS = (1, 3, 6, 9, 12)
TAP_CHANNELS = (64, 128, 256, 512, 512)
MEAN = (-.030, -.088, -.188)
STD = (.458, .448, .450)
EPS = 1e-10
_M64 = (1 << 64) - 1


def hash_uniform(seed: int, stream: int, n: int) -> np.ndarray:
    """n doubles in [0, 1): splitmix64 of the counter, offset by (seed, stream)."""
    off = (seed * 0x9E3779B97F4A7C15 + stream * 0xD1B54A32D192ED03 + 0x2545F4914F6CDD1D) & _M64
    z = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(off)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def seeded_weights(seed: int) -> dict:
    """State dict (fp32 tensors, the reference's key names): conv weights uniform in +-sqrt(6 / (9 Cin)), biases in +-0.05, lin weights
    non-negative with mean 1 / C."""
    sd = {"net.mean": torch.tensor(MEAN, dtype=torch.float32)[None, :, None, None],
          "net.std": torch.tensor(STD, dtype=torch.float32)[None, :, None, None]}
    for k, (i, cin, cout) in enumerate(VGG_CONVS):
        w = (hash_uniform(seed, 2 * k, cout * cin * 9) * 2 - 1) * np.sqrt(6.0 / (9 * cin))
        b = (hash_uniform(seed, 2 * k + 1, cout) * 2 - 1) * 0.05
        sd[f"net.layers.{i}.weight"] = torch.from_numpy(w.reshape(cout, cin, 3, 3)).float()
        sd[f"net.layers.{i}.bias"] = torch.from_numpy(b).float()
    for t, c in enumerate(TAP_CHANNELS):
        sd[f"lin.{t}.1.weight"] = torch.from_numpy(hash_uniform(seed, 100 + t, c) * 2.0 / c).float().reshape(1, c, 1, 1)
    return sd


def seeded_images(seed: int, shape, noise: float = 0.1):
    """(x, y) fp32 in [-1, 1]: y = the prediction plus noise, clipped."""
    n = int(np.prod(shape))
    x = hash_uniform(seed, 1000, n) * 2 - 1
    y = np.clip(x + (hash_uniform(seed, 1001, n) * 2 - 1) * noise, -1, 1)
    return torch.from_numpy(x.reshape(shape)).float(), torch.from_numpy(y.reshape(shape)).float()


# ---- the composition (NCHW, any floating dtype; the reference's formulas) -------------------------------------------------------------

def trunk(x: torch.Tensor, sd: dict, dtype=torch.float64):
    """The 13 ReLU outputs (NCHW) of the z-scored image."""
    a = (x.to(dtype) - sd["net.mean"].to(dtype)) / sd["net.std"].to(dtype)
    acts = []
    for k, (i, _, _) in enumerate(VGG_CONVS):
        a = F.relu(F.conv2d(a, sd[f"net.layers.{i}.weight"].to(dtype), sd[f"net.layers.{i}.bias"].to(dtype), padding=1))
        acts.append(a)
        if k in POOL_AFTER:
            a = F.max_pool2d(a, 2, 2)
    return acts


def normalize(a: torch.Tensor) -> torch.Tensor:
    return a / (torch.sqrt(torch.sum(a ** 2, dim=1, keepdim=True)) + EPS)


def lpips(x: torch.Tensor, y: torch.Tensor, sd: dict, dtype=torch.float64) -> torch.Tensor:
    ax, ay = trunk(x, sd, dtype), trunk(y, sd, dtype)
    total = 0.0
    for t, k in enumerate(TAPS):
        d = (normalize(ax[k]) - normalize(ay[k])) ** 2
        total = total + (d * sd[f"lin.{t}.1.weight"].to(d.dtype)).sum(1, keepdim=True).mean((2, 3), True).sum()
    return total / x.shape[0]


def loss_and_grad(x, y, sd, dtype=torch.float64, autocast=None):
    """(loss, d loss / d x) as float64 tensors; autocast: a dtype for torch.autocast('cpu') around an fp32 composition."""
    xr = x.to(dtype).clone().requires_grad_(True)
    if autocast is not None:
        with torch.autocast("cpu", dtype=autocast):
            l = lpips(xr, y.to(dtype), sd, dtype)
    else:
        l = lpips(xr, y.to(dtype), sd, dtype)
    l.backward()
    return l.detach().double(), xr.grad.double()


# ---- per-stage references: NHWC tensors as the kernels store them ---------------------------------------------------------------------

def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def conv_model(a16, w16, bias=None, addend=None, mask_src=None, relu=False):
    """(reference, bound), float64 NHWC, of gvf_conv3x3 on the 16-bit operands a16 (N,H,W,Cin) and w16 (Cout,Cin,3,3) -- for the input-
    gradient direction pass the flipped, transposed weight (dgrad_weight).  ceil(9 Cin / 32) k-steps (module docstring)."""
    dt = a16.dtype
    a, w = nchw(a16.double()), w16.double()
    pre = nhwc(F.conv2d(a, w, padding=1))
    S = nhwc(F.conv2d(a.abs(), w.abs(), padding=1))
    other = torch.zeros_like(pre)
    if bias is not None:
        pre, other = pre + bias.double(), other + bias.double().abs()
    e = accumulation_error(9 * a16.shape[3], S, other)
    if addend is not None:
        e = e + U32 * (S + other + addend.double().abs())
        pre = pre + addend.double()
    if relu:
        pre = F.relu(pre)
    bnd = _round_bound(pre, e, dt)
    if mask_src is not None:
        m = (mask_src.double() > 0).double()
        pre, bnd = pre * m, bnd * m
    return pre, bnd


def dgrad_weight(w: torch.Tensor) -> torch.Tensor:
    """(Cout,Cin,3,3) -> the (Cin,Cout,3,3) weight whose pad-1 convolution is the input gradient: taps flipped, channel roles swapped."""
    return w.flip(2, 3).transpose(0, 1).contiguous()


def first_operand(x: torch.Tensor, dt) -> torch.Tensor:
    """The first layer's 16-bit operand (N,H,W,3): the fp32 z-score (one subtraction, one division, as the kernel) rounded to dt."""
    z = (x.float() - torch.tensor(MEAN)[None, :, None, None]) / torch.tensor(STD)[None, :, None, None]
    return nhwc(z).to(dt)


def first_backward_model(z16, w):
    """(reference, bound) fp64 NCHW of gvf_lpips_first_backward: z16 (N,H,W,64) bf16, w fp32 (64,3,3,3)."""
    z, wd = nchw(z16.double()), dgrad_weight(w.double())
    std = torch.tensor(STD, dtype=torch.float64)[None, :, None, None]
    ref = F.conv2d(z, wd, padding=1) / std
    S = F.conv2d(z.abs(), wd.abs(), padding=1) / std
    return ref, (9 * 64 + 2) * U32 * S + U32 * ref.abs()


def pool_route(a16):
    """(pooled (N,H/2,W/2,C) in a16's dtype, mine (N,H,W,C) bool): the 2x2 / 2 floor max pool and, per element, whether it is the FIRST
    maximum of its window in row-major order (False on rows and columns the floor drops)."""
    N, H, W, C = a16.shape
    Ho, Wo = H // 2, W // 2
    win = a16[:, :2 * Ho, :2 * Wo].double().reshape(N, Ho, 2, Wo, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(N, Ho, Wo, C, 4)
    idx = torch.argmax(win, dim=-1)                    # the first maximal value's index
    pooled = torch.gather(win, -1, idx[..., None])[..., 0].to(a16.dtype)
    onehot = F.one_hot(idx, 4).bool().reshape(N, Ho, Wo, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(N, 2 * Ho, 2 * Wo, C)
    mine = torch.zeros((N, H, W, C), dtype=torch.bool)
    mine[:, :2 * Ho, :2 * Wo] = onehot
    return pooled, mine


def pool_backward_model(a16, g_pooled, tap_grad):
    """(reference, bound) fp64 of gvf_maxpool2x2_backward: one fp32 add, rounded to bf16."""
    _, mine = pool_route(a16)
    g = g_pooled.double().repeat_interleave(2, 1).repeat_interleave(2, 2)
    gfull = torch.zeros_like(tap_grad, dtype=torch.float64)
    gfull[:, :g.shape[1], :g.shape[2]] = g
    v = torch.where(mine, gfull, torch.zeros_like(gfull)) + tap_grad.double()
    e = torch.where(mine, U32 * v.abs(), torch.zeros_like(v))
    m = (a16.double() > 0).double()
    return v * m, _round_bound(v, e, torch.bfloat16) * m


def tap_terms(ax, ay, lin, dtype=torch.float64):
    """The N per-image terms of one tap from stored activations (N,H,W,C), evaluated in `dtype` with the reference's formula."""
    a, b, l = ax.to(dtype), ay.to(dtype), lin.to(dtype)
    u = a / (torch.sqrt((a * a).sum(-1, keepdim=True)) + EPS)
    v = b / (torch.sqrt((b * b).sum(-1, keepdim=True)) + EPS)
    return (((u - v) ** 2) * l).sum(-1).mean((1, 2))


def tap_grad(ax, ay, lin, upstream, dtype=torch.float64):
    """upstream[n] d term[n] / d ax in `dtype`, the closed form of gvf_lpips.h (a_k / |a| = 0 on an all-zero pixel)."""
    a, b, l = ax.to(dtype), ay.to(dtype), lin.to(dtype)
    r = torch.sqrt((a * a).sum(-1, keepdim=True))
    D = r + EPS
    u = a / D
    v = b / (torch.sqrt((b * b).sum(-1, keepdim=True)) + EPS)
    hw = a.shape[1] * a.shape[2]
    w = 2 * upstream.to(dtype)[:, None, None, None] * l * (u - v) / hw
    dot = (w * u).sum(-1, keepdim=True)
    dirn = torch.where(r > 0, a / torch.where(r > 0, r, torch.ones_like(r)), torch.zeros_like(a))
    return (w - dirn * dot) / D
