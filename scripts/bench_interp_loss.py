"""Fused KNN interpolation loss (ops/knn_interp.py: search + weights, fused gather + L1, gradient) against the same loss composed in
torch (the encoder's compute_delta_interp: a (B, L, N, 3) broadcast difference, the (B, L, N) distance matrix, topk; then the masked L1
with autograd backward), forward + backward, at the training shape (1, 262144, 8192, 24, 8) -- where the composition runs in query
chunks of 32 768, as it cannot hold the full distance matrix beside its broadcast differences -- and at the encoder shape
(8, 512, 8192, 24, 8) (the estimate alone: the encoder takes no loss).  GPU only.  The two sides alternate in one process; device
events around GVF_STEPS timed calls per side (default 20) after a warm-up.  Prints ms, the ratio, and the achieved rates of the search
and of the loss kernels against their counted work."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gvfdiffusion_amd.model.autoencoder import GSKLTemporalVariationalAutoEncoder as VAE  # noqa: E402
from gvfdiffusion_amd.ops import knn_interp as KI  # noqa: E402

dev = torch.device("cuda:0")
N_STEPS = int(os.environ.get("GVF_STEPS", 20))
ROUNDS = 4                                         # fused / composed alternate ROUNDS times, N_STEPS / ROUNDS calls each
CHUNK = 32768

# counted work (csrc/interp.hip)
#   search: 9 VALU operations per (query, anchor) pair without contraction (3 sub, 3 mul, 2 add, 1 compare); the fp32 vector peak of
#           157.3 TFLOP/s counts an fma as two, so it is 78.6 T operations/s for these: 8.7 T pairs/s.
#   loss forward + backward, per (b, t, p) row: pred read through its 14-channel rows (56 B: whole lines are fetched), 1 sign byte
#           written and read, the 14-channel gradient row written (56 B); per (b, p): idx + w read (8 K B).  The K gathered anchor
#           rows per (b, t, p) (12 K B) come from the 2.4 MB table of the sample in L2 and are not HBM traffic.
OPS_PAIR, VALU_OPS_PEAK, HBM_PEAK = 9, 78.6e12, 6.3e12


def inputs(B, P, N, T, C=14, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = (torch.rand((B, P, 3), generator=g) - 0.5).to(dev)
    a = (torch.rand((B, N, 3), generator=g) - 0.5).to(dev)
    m = a[:, None] + 0.05 * torch.randn((B, T, N, 3), generator=g).to(dev)
    pred = (0.05 * torch.randn((B, T, P, C), generator=g)).to(dev)
    return q, a, m, pred


def timed_pair(f0, f1, n):
    """ms per call of f0 and of f1: ROUNDS alternating windows of n / ROUNDS calls each, after one warm-up call of both."""
    f0(); f1()
    torch.cuda.synchronize()
    per = max(1, n // ROUNDS)
    tot = [0.0, 0.0]
    for _ in range(ROUNDS):
        for i, f in enumerate((f0, f1)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(per):
                f()
            e1.record()
            torch.cuda.synchronize()
            tot[i] += e0.elapsed_time(e1)
    return tot[0] / (per * ROUNDS), tot[1] / (per * ROUNDS)


def composed_est(q, a, m, k):
    P = q.shape[1]
    return torch.cat([VAE.compute_delta_interp(q[:, p0:p0 + CHUNK], a, m, knn_k=k) for p0 in range(0, P, CHUNK)], dim=2)


def main():
    B, P, N, T, K = 1, int(os.environ.get("GVF_P", 262144)), 8192, 24, 8
    q, a, m, pred = inputs(B, P, N, T)
    pred.requires_grad_(True)

    def fused():
        pred.grad = None
        KI.interpolation_l1(pred, q, a, m, k=K).backward()

    def composed():
        pred.grad = None
        est = composed_est(q, a, m, K)
        torch.abs(pred[..., :3] - est).sum().div(3.0 * T * B * P).backward()

    with torch.no_grad():
        idx, w = KI.knn_interp_weights(q, a, k=K)

    def search():
        KI.knn_interp_weights(q, a, k=K)

    def loss_only():
        pred.grad = None
        KI._InterpL1Fn.apply(pred, idx, w, a, m, None, False)[0].backward()

    tf, tc = timed_pair(fused, composed, N_STEPS)
    ts, tl = timed_pair(search, loss_only, N_STEPS)
    with torch.no_grad():
        lf, lc = float(KI.interpolation_l1(pred, q, a, m, k=K)), float(torch.abs(pred[..., :3] - composed_est(q, a, m, K)).sum() / (3.0 * T * B * P))
    pairs = B * P * N
    loss_bytes = B * T * P * (56 + 1 + 1 + 56) + B * P * K * 8
    print(f"interpolation loss ({B}, {P}, {N}, {T}, {K}), forward + backward: fused {tf:.3f} ms, torch-composed (query chunks of {CHUNK}) "
          f"{tc:.2f} ms, {tc / tf:.1f}x; loss fused {lf:.9g} composed {lc:.9g}", flush=True)
    print(f"  search + weights {ts:.3f} ms: {pairs / ts / 1e9:.2f} T pairs/s = {OPS_PAIR * pairs / ts / 1e9 / (VALU_OPS_PEAK / 1e12) * 100:.1f} % of the "
          f"fp32 VALU rate at {OPS_PAIR} operations per pair (compute-bound: its bytes are negligible)", flush=True)
    print(f"  loss forward + backward {tl:.3f} ms: {loss_bytes / tl / 1e9:.2f} TB/s of {loss_bytes / 1e6:.0f} MB counted HBM bytes = "
          f"{loss_bytes / tl / 1e9 / (HBM_PEAK / 1e12) * 100:.1f} % of 6.3 TB/s (memory-bound)", flush=True)
    del q, a, m, pred, idx, w

    B, P = 8, 512
    q, a, m, _ = inputs(B, P, N, T, seed=1)
    te, tt = timed_pair(lambda: VAE.compute_delta_interp(q, a, m, knn_k=K, fused=True), lambda: VAE.compute_delta_interp(q, a, m, knn_k=K), N_STEPS)
    print(f"encoder estimate ({B}, {P}, {N}, {T}, {K}): compute_delta_interp fused=True {te:.3f} ms, torch path {tt:.3f} ms, {tt / te:.1f}x "
          "(reported only)", flush=True)


if __name__ == "__main__":
    main()
