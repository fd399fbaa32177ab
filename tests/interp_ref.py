"""References, error bounds and input generators for the KNN interpolation loss tests (include/gvf_interp.h, rules 1-5).

(i)   `interp_ref64`: a float64 restatement of the rules with a stable order among equal distances, in torch so that it runs where its
      inputs live (CPU in the host tests, the device for the large cases) and in query chunks (no full (P, N) matrix).  Besides the
      results it returns, per query, the two decision margins
          gap    = (d_{K+1} - d_K) / max(d_{K+1}, 1e-30)      (infinite when N = K): how far the K-th place is from changing hands,
          margin = min_k |d_k - r2| / r2                      (adaptive only, else infinite): how far a weight is from being cut.
      A query whose margins are below the test's threshold may legitimately decide differently in fp32; above it, it may not.
(ii)  `interp_torch32`: the fp32 torch composition (the encoder's compute_delta_interp plus the masked L1), the yardstick.
(iii) `dist_bound`, `weight_bound`, `estimate_bound`: element-wise bounds of an fp32 evaluation against (i), derived from the
      operation sequence (not fitted).  u = 2^-24 is the unit roundoff; every fp32 operation (+, -, *, /, sqrt) is correctly rounded
      (relative error <= u) and expf is taken to be within 2 ulp (<= 4 u).  Inputs are fp32 numbers, so (i) starts from the same values.

      d:    dx = fl(qx - ax) carries u, fl(dx dx) 3 u in all; the terms are non-negative, so the two additions add at most u each
            relative to the sum: |d32 - d64| <= 5 u d64 to first order                                      -> dist_bound = 6 u d64.
      r2:   the mean of K non-negative d_k: 5 u from d, at most (K - 1) u from the additions (any order), u from the division:
            (K + 5) u.  sqrt halves it and adds u; the constant 1e-6 is rounded to fp32 (u relative to itself, less relative to r)
            and added (u): r carries ((K + 5) / 2 + 3) u.  r2 = fl(r r): twice that plus u = (K + 12) u.
      x:    the exponent's argument x_k = beta d_k / r2 (adaptive; beta d_k otherwise) is formed by one multiplication and one
            division on d_k (5 u) and r2: at most (K + 19) u relative (the non-adaptive form is smaller: 6 u).  A relative error e
            of x is an absolute error x e of the exponent, i.e. a relative error x e of exp(x); expf adds 4 u:
            e_k = (x_k (K + 19) + 4) u for the unnormalised weight.  A neighbour cut by the radius has weight 0 exactly
            (that decision is guarded by `margin`).
      w:    S = sum_k w_k + 1e-8: a sum of non-negative terms, so its relative error is at most max_k e_k over the kept neighbours,
            plus (K - 1) u for the additions, u for the constant's rounding and u for adding it.  The division adds u:
            |w32 - w64| <= (e_k + max_j e_j + (K + 2) u) w64 <= c_w u w64,   c_w = 2 X (K + 19) + K + 10,  X = max_kept x_j
            (not adaptive: c_w = 2 X 6 + K + 10).
            At beta = 7, K = 8, adaptive (X <= 7): c_w <= 396.
      est:  each term fl(w_k fl(m_k - a_k)) carries c_w u + 2 u relative to |w_k (m_k - a_k)|, the K - 1 additions at most (K - 1) u
            relative to sum_k |w_k (m_k - a_k)|:  |est32 - est64| <= (c_w + K + 1) u sum_k w_k |m_k - a_k|  per component.
      Second-order terms are below 1e-4 of these (c u < 1e-4), covered by the factor 1.01; 1e-37 absorbs the subnormal range.
"""
import math
import os

import numpy as np
import torch

U = 2.0 ** -24
SLACK = 1.01
TINY = 1e-37


def _lengths(lengths, B, P):
    return [P] * B if lengths is None else [int(v) for v in lengths]


def _stable_topk(d, kk):
    """(Q, N) float64 -> values, indices of the kk smallest per row, ascending, the lower index first among equal values."""
    vals, idx = torch.topk(d, kk, dim=1, largest=False, sorted=True)
    tie = (d == vals[:, -1:]).sum(dim=1) > 1
    if kk > 1:
        tie |= (vals[:, 1:] == vals[:, :-1]).any(dim=1)
    rows = torch.nonzero(tie).flatten()
    if rows.numel():
        order = torch.argsort(d[rows], dim=1, stable=True)[:, :kk]
        idx[rows] = order
        vals[rows] = torch.gather(d[rows], 1, order)
    return vals, idx


def interp_ref64(q, a, m, lengths=None, k=8, beta=7.0, adaptive=True, pred=None, chunk=2048):
    """Rules 1-5 in float64.  q (B, P, 3), a (B, N, 3), m (B, T, N, 3), pred (B, T, P, >= 3) or None: fp32 or float64 tensors.
    Returns a dict of float64 / int64 tensors: idx, dist, w (B, P, K); gap, margin, xmax (B, P); est, est_abs (B, T, P, 3)
    (est_abs = sum_k w_k |m_k - a_k|); movmax (B, T, P) = max_k,c |m_k - a_k|; and with pred: loss (0-d), grad (B, T, P, 3)."""
    q, a, m = q.double(), a.double(), m.double()
    B, P, N, T = q.shape[0], q.shape[1], a.shape[1], m.shape[1]
    lens = _lengths(lengths, B, P)
    beta = float(np.float32(beta))
    dev = q.device
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=dev)  # noqa: E731
    out = {"idx": z(B, P, k, dt=torch.int64), "dist": z(B, P, k), "w": z(B, P, k), "gap": z(B, P), "margin": z(B, P), "xmax": z(B, P),
           "est": z(B, T, P, 3), "est_abs": z(B, T, P, 3), "movmax": z(B, T, P)}
    kk = k + 1 if N > k else k
    for b in range(B):
        for p0 in range(0, lens[b], chunk):
            p1 = min(lens[b], p0 + chunk)
            qc = q[b, p0:p1]
            dx = qc[:, None, 0] - a[b, None, :, 0]
            d = dx * dx
            dx = qc[:, None, 1] - a[b, None, :, 1]
            d += dx * dx
            dx = qc[:, None, 2] - a[b, None, :, 2]
            d += dx * dx
            vals, idx = _stable_topk(d, kk)
            del d, dx
            dk, ik = vals[:, :k], idx[:, :k]
            gap = (vals[:, k] - vals[:, k - 1]) / vals[:, k].clamp_min(1e-30) if kk > k else torch.full_like(vals[:, 0], math.inf)
            r = dk.mean(dim=1).sqrt() + 1e-6
            r2 = (r * r)[:, None]
            if adaptive:
                x = beta * dk / r2
                keep = dk <= r2
                w = torch.exp(-x) * keep
                margin = ((dk - r2).abs() / r2).min(dim=1).values
            else:
                x = beta * dk
                keep = torch.ones_like(dk, dtype=torch.bool)
                w = torch.exp(-x)
                margin = torch.full_like(gap, math.inf)
            w = w / (w.sum(dim=1, keepdim=True) + 1e-8)
            mov = m[b][:, ik] - a[b][ik][None]                       # (T, Q, K, 3)
            out["idx"][b, p0:p1], out["dist"][b, p0:p1], out["w"][b, p0:p1] = ik, dk, w
            out["gap"][b, p0:p1], out["margin"][b, p0:p1] = gap, margin
            out["xmax"][b, p0:p1] = torch.where(keep, x, torch.zeros_like(x)).max(dim=1).values
            out["est"][b, :, p0:p1] = (mov * w[None, :, :, None]).sum(dim=2)
            out["est_abs"][b, :, p0:p1] = (mov.abs() * w[None, :, :, None]).sum(dim=2)
            out["movmax"][b, :, p0:p1] = mov.abs().amax(dim=(2, 3))
        out["gap"][b, lens[b]:] = math.inf
        out["margin"][b, lens[b]:] = math.inf
    if pred is not None:
        cnt = 3.0 * T * sum(lens)
        mask = torch.zeros((B, 1, P, 1), dtype=torch.float64, device=dev)
        for b in range(B):
            mask[b, :, :lens[b]] = 1.0
        diff = (pred[..., :3].double() - out["est"]) * mask
        out["loss"] = diff.abs().sum() / cnt
        out["grad"] = torch.sign(diff) / cnt
    return out


def interp_torch32(q, a, m, lengths=None, k=8, beta=7.0, adaptive=True, pred=None, chunk=None):
    """The fp32 torch composition: the encoder's compute_delta_interp (brute-force topk over the distance matrix, in query chunks of
    `chunk` if given) and the reference's masked L1.  Returns {"est" (padded rows zeroed)[, "loss", "grad"]}."""
    from gvfdiffusion_amd.model.autoencoder import GSKLTemporalVariationalAutoEncoder as VAE
    q, a, m = q.float(), a.float(), m.float()
    B, P, T = q.shape[0], q.shape[1], m.shape[1]
    lens = _lengths(lengths, B, P)
    step = P if chunk is None else chunk
    est = torch.cat([VAE.compute_delta_interp(q[:, p0:p0 + step], a, m, knn_k=k, beta=beta, adaptive_radius=adaptive)
                     for p0 in range(0, P, step)], dim=2)
    mask = torch.arange(P, device=q.device)[None, :] < torch.tensor(lens, device=q.device)[:, None]            # (B, P)
    est = est * mask[:, None, :, None]
    out = {"est": est}
    if pred is not None:
        pr = pred.detach().float().clone().requires_grad_(True)
        mk = mask[:, None, :].expand(B, T, P)
        loss = (torch.abs(pr[..., :3] - est) * mk.unsqueeze(-1)).sum() / (mk.sum() * 3)
        loss.backward()
        out["loss"], out["grad"] = loss.detach(), pr.grad
    return out


def dist_bound(ref):
    return 6.0 * U * ref["dist"] + TINY


def weight_constant(ref, k, adaptive=True):
    """c_w per query (B, P): 2 X e_x + K + 10 with e_x = K + 19 (adaptive) or 6 (not adaptive), see the module docstring."""
    return 2.0 * ref["xmax"] * ((k + 19) if adaptive else 6) + k + 10


def weight_bound(ref, k, adaptive=True):
    return SLACK * U * weight_constant(ref, k, adaptive)[..., None] * ref["w"] + TINY


def estimate_bound(ref, k, adaptive=True):
    c = weight_constant(ref, k, adaptive) + k + 1                                   # (B, P)
    return SLACK * U * c[:, None, :, None] * ref["est_abs"] + TINY


# ---- seeded inputs (CPU generators, so that every machine sees the same numbers) ---------------------------------------------------
def make_case(seed, lens, N, T, C=3, pred_noise=0.02, scale=1.0):
    """A uniform cloud in scale * [-0.5, 0.5]^3 with B = len(lens) samples, P = max(lens) query slots, motion ~ 0.05 scale randn;
    padded query slots hold zeros (as the reference pads them).  Returns q, a, m fp32 and a noise tensor (B, T, P, C) ~ pred_noise
    scale randn for pred = est + noise."""
    g = torch.Generator().manual_seed(seed)
    B, P = len(lens), max(lens)
    q = scale * (torch.rand((B, P, 3), generator=g) - 0.5)
    for b, n in enumerate(lens):
        q[b, n:] = 0.0
    a = scale * (torch.rand((B, N, 3), generator=g) - 0.5)
    m = a[:, None] + 0.05 * scale * torch.randn((B, T, N, 3), generator=g)
    noise = pred_noise * scale * torch.randn((B, T, P, C), generator=g)
    return q, a, m, noise


# The case matrix of the device tests (B and P from `lens`).  FLAG = 1e-5 is the decision threshold on gap and margin.  For the cases
# with P <= 1000 the seeds are ones for which the float64 reference flags no query, adaptive or not (asserted by the tests).
# "k1": with K = 1 the radius is r2 = (sqrt(d) + 1e-6)^2, so margin = (r2 - d) / r2 ~ 2e-6 / sqrt(d) by construction: in a unit cube
# with 70 anchors a tenth of the queries has sqrt(d) > 0.2 and would fall under the threshold, so this cloud is a quarter the size
# (sqrt(d) < 0.1 throughout; both margins are relative, so nothing else changes with the scale).
FLAG = 1e-5
CASES = {
    "one": dict(seed=1, lens=[1], N=8, T=1, k=8),
    "ragged2": dict(seed=2, lens=[150, 97], N=300, T=5, k=8),
    "large": dict(seed=3, lens=[20000], N=8192, T=4, k=8),
    "ragged3": dict(seed=4, lens=[4097, 64, 1], N=512, T=24, k=4),
    "k16": dict(seed=5, lens=[5000], N=4096, T=2, k=16),
    "k1": dict(seed=6, lens=[1000], N=70, T=3, k=1, scale=0.25),
}
SMALL_CASES = ("one", "ragged2", "k1")        # P <= 1000: no flagged query


def case_inputs(name, C=3):
    c = CASES[name]
    return make_case(c["seed"], c["lens"], c["N"], c["T"], C=C, scale=c.get("scale", 1.0))


def unflagged(ref, lens):
    """(B, P) bool: valid queries whose two decision margins both exceed FLAG; and the valid mask."""
    B, P = ref["gap"].shape
    valid = torch.arange(P, device=ref["gap"].device)[None, :] < torch.tensor(list(lens), device=ref["gap"].device)[:, None]
    return valid & (ref["gap"] > FLAG) & (ref["margin"] > FLAG), valid


def lattice_case(seed=11, P=256, half=40, T=3):
    """Exact ties: coordinates are multiples of 1/64 in [-0.5, 0.5], so every squared distance is exact in fp32 and in float64 alike;
    the anchors are `half` lattice points, each present twice (index i and half + i) with different motions, so every distance
    comes at least in pairs and an odd K splits a pair at the K-th place."""
    g = torch.Generator().manual_seed(seed)
    lat = lambda *s: torch.randint(-32, 33, s, generator=g).float() / 64.0  # noqa: E731
    q = lat(1, P, 3)
    base = lat(1, half, 3)
    a = torch.cat([base, base], dim=1)
    m = a[:, None] + 0.05 * torch.randn((1, T, 2 * half, 3), generator=g)
    return q, a, m


# ---- the recorded results of the reference (tests/golden/make_interp_golden.py) ----------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "interp_loss_golden.npz")
ENCODE_GOLDEN = os.path.join(ROOT, "tests", "golden", "vae_encode_golden.npz")
GOLDEN_CASES = ("base", "fixed_radius", "k4", "n_eq_k")


# Elements of a recorded case whose output lies within the estimate bound of the float64 estimate, so that the sign of an fp32
# evaluation is not determined there (a property of the fixture alone, asserted on the CPU by test_interp_ref): one in `n_eq_k`,
# element (1, 2, 10, 2), |output - est64| = 3.2e-7 under a bound of 1.2e-6.
GOLDEN_UNDER_BOUND = {"base": 0, "fixed_radius": 0, "k4": 0, "n_eq_k": 1}


def golden_sure(name, ref, valid, output, est64, k, adaptive):
    """(B, T, P, 3) bool: the valid elements of a recorded case whose gradient sign is determined; their complement among the valid
    elements has exactly GOLDEN_UNDER_BOUND[name] members."""
    sure = (output[..., :3].double() - est64).abs() > estimate_bound(ref, k, adaptive)
    sure = sure & valid[:, None, :, None]
    n_el = int(valid.sum()) * 3 * output.shape[1]
    assert n_el - int(sure.sum()) == GOLDEN_UNDER_BOUND[name], (name, n_el - int(sure.sum()))
    return sure


def golden_case(name):
    """-> gs list, static_pc, moving_pc, output, k, adaptive, beta, and the recorded arrays of the case as a dict."""
    z = np.load(GOLDEN)
    s = str(z[f"{name}.input_set"])
    gs = []
    while f"in.{s}.gs{len(gs)}" in z.files:
        gs.append(torch.from_numpy(z[f"in.{s}.gs{len(gs)}"]))
    k, adaptive, beta = z[f"{name}.params"]
    rec = {key.split(".", 1)[1]: z[key] for key in z.files if key.startswith(name + ".")}
    return (gs, torch.from_numpy(z[f"in.{s}.static_pc"]), torch.from_numpy(z[f"in.{s}.moving_pc"]), torch.from_numpy(z[f"in.{s}.output"]),
            int(k), bool(adaptive), float(beta), rec)


def padded_queries(gs):
    P = max(g.shape[0] for g in gs)
    return torch.stack([torch.nn.functional.pad(g[:, :3], (0, 0, 0, P - g.shape[0])) for g in gs]), [g.shape[0] for g in gs]
