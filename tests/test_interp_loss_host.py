"""Host side of the KNN interpolation loss (include/gvf_interp.h): every entry point refuses bad arguments before any launch, the
scratch size does not depend on the anchors, and the Python entry points refuse CPU tensors and inconsistent inputs.  No GPU needed."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def L():
    from gvfdiffusion_amd import _lib
    from gvfdiffusion_amd.ops import knn_interp  # noqa: F401  (registers the signatures)
    return _lib.lib()


X = ctypes.c_void_p(256)       # a non-null "device pointer": every call below is refused before anything could read it


def weights(L, q=X, a=X, idx=X, w=X, B=1, P=4, N=8, K=4):
    return L.gvf_knn_interp_weights(q, None, a, B, P, N, K, 7.0, 1, idx, w, None, None)


def apply_(L, idx=X, w=X, a=X, m=X, est=X, B=1, T=2, P=4, N=8, K=4):
    return L.gvf_knn_interp_apply(idx, w, a, m, B, T, P, N, K, est, None)


def forward(L, pred=X, stride=3, idx=X, w=X, a=X, m=X, loss=X, scratch=X, nbytes=1 << 20, B=1, T=2, P=4, N=8, K=4):
    return L.gvf_interp_loss_forward(pred, stride, idx, w, a, m, None, B, T, P, N, K, loss, None, None, scratch, nbytes, None)


def backward(L, sign=X, g=X, grad=X, stride=3, ch=3, B=1, T=2, P=4):
    return L.gvf_interp_loss_backward(sign, g, None, B, T, P, grad, stride, ch, None)


def test_weights_refusals(L):
    from gvfdiffusion_amd._lib import GVF_EINVAL
    for kw in [dict(q=None), dict(a=None), dict(idx=None), dict(w=None), dict(K=0), dict(K=17, N=32), dict(K=5, N=4), dict(B=0), dict(P=0),
               dict(N=0), dict(B=-1), dict(P=-4)]:
        assert weights(L, **kw) == GVF_EINVAL, kw


def test_apply_refusals(L):
    from gvfdiffusion_amd._lib import GVF_EINVAL
    for kw in [dict(idx=None), dict(w=None), dict(a=None), dict(m=None), dict(est=None), dict(K=0), dict(K=17, N=32), dict(K=9, N=8),
               dict(B=0), dict(T=0), dict(P=0), dict(N=-1)]:
        assert apply_(L, **kw) == GVF_EINVAL, kw


def test_loss_forward_refusals(L):
    from gvfdiffusion_amd._lib import GVF_EINVAL, GVF_ENOSPC
    for kw in [dict(pred=None), dict(idx=None), dict(w=None), dict(a=None), dict(m=None), dict(loss=None), dict(scratch=None),
               dict(stride=2), dict(stride=0), dict(stride=-3), dict(K=0), dict(K=17, N=32), dict(K=9, N=8), dict(B=0), dict(T=0),
               dict(P=-1), dict(N=0)]:
        assert forward(L, **kw) == GVF_EINVAL, kw
    need = ctypes.c_size_t(0)
    assert L.gvf_interp_loss_scratch_bytes(1, 2, 4, ctypes.byref(need)) == 0 and need.value >= 8
    assert forward(L, nbytes=need.value - 1) == GVF_ENOSPC
    assert forward(L, nbytes=0) == GVF_ENOSPC


def test_loss_backward_refusals(L):
    from gvfdiffusion_amd._lib import GVF_EINVAL
    for kw in [dict(sign=None), dict(g=None), dict(grad=None), dict(stride=2), dict(ch=2), dict(ch=4, stride=3), dict(ch=15, stride=14),
               dict(B=0), dict(T=-1), dict(P=0)]:
        assert backward(L, **kw) == GVF_EINVAL, kw


def test_scratch_bytes(L):
    from gvfdiffusion_amd._lib import GVF_EINVAL
    out = ctypes.c_size_t(0)
    assert L.gvf_interp_loss_scratch_bytes(1, 24, 262144, ctypes.byref(out)) == 0
    full = out.value
    assert 8 * 1024 <= full <= 1 << 20                  # a double per workgroup: nothing per query, per frame or per anchor
    # the signature has no N or K at all: the scratch cannot grow with the anchors.  It grows with the query blocks only.
    assert L.gvf_interp_loss_scratch_bytes(8, 24, 512, ctypes.byref(out)) == 0 and 0 < out.value <= 1 << 20
    assert L.gvf_interp_loss_scratch_bytes(1, 1, 1, ctypes.byref(out)) == 0 and out.value >= 8
    for args in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1), (70000, 1, 1), (1 << 15, 1 << 30, 1 << 30)]:
        assert L.gvf_interp_loss_scratch_bytes(*args, ctypes.byref(out)) == GVF_EINVAL, args
    assert L.gvf_interp_loss_scratch_bytes(1, 1, 1, None) == GVF_EINVAL


def _clouds(B=2, P=10, N=20, T=3, C=14):
    g = torch.Generator().manual_seed(0)
    return (torch.rand((B, P, 3), generator=g), torch.rand((B, N, 3), generator=g), torch.rand((B, T, N, 3), generator=g),
            torch.rand((B, T, P, C), generator=g))


def test_operators_refuse_cpu_tensors():
    from gvfdiffusion_amd import _lib, training
    from gvfdiffusion_amd.ops import knn_interp as KI
    from gvfdiffusion_amd.model.autoencoder import GSKLTemporalVariationalAutoEncoder as VAE
    q, a, m, pred = _clouds()
    with pytest.raises(_lib.GvfError):
        KI.knn_interp_weights(q, a)
    with pytest.raises(_lib.GvfError):
        KI.delta_interp(q, a, m, lengths=[10, 7])
    with pytest.raises(_lib.GvfError):
        KI.interpolation_l1(pred, q, a, m)
    with pytest.raises(_lib.GvfError):
        training.interpolation_loss([q[0], q[1, :7]], a, m, pred)
    with pytest.raises(_lib.GvfError):
        VAE.compute_delta_interp(q, a, m, fused=True)
    assert VAE.compute_delta_interp(q, a, m).shape == (2, 3, 10, 3)          # the default path is the torch composition, CPU included


def test_operators_refuse_inconsistent_inputs():
    from gvfdiffusion_amd import training
    from gvfdiffusion_amd.ops import knn_interp as KI
    q, a, m, pred = _clouds()
    bad = [
        lambda: KI.knn_interp_weights(q[..., :2], a),                          # not xyz
        lambda: KI.knn_interp_weights(q, a[:1]),                               # sample counts differ
        lambda: KI.knn_interp_weights(q, a, k=21),                             # K > N
        lambda: KI.knn_interp_weights(q, a, k=17),                             # K > 16
        lambda: KI.knn_interp_weights(q, a, k=0),
        lambda: KI.knn_interp_weights(q, a, lengths=[10, 11]),                 # a length above P
        lambda: KI.knn_interp_weights(q, a, lengths=torch.tensor([10, 11])),
        lambda: KI.knn_interp_weights(q, a, lengths=[10]),
        lambda: KI.knn_interp_weights(q, a, lengths=[-1, 3]),
        lambda: KI.delta_interp(q, a, m[:, :, :19]),                           # anchors differ
        lambda: KI.delta_interp(q, a, m[:1]),
        lambda: KI.delta_interp(q.clone().requires_grad_(True), a, m),         # differentiable in pred only
        lambda: KI.interpolation_l1(pred, q, a.clone().requires_grad_(True), m),
        lambda: KI.interpolation_l1(pred, q, a, m.clone().requires_grad_(True)),
        lambda: KI.interpolation_l1(pred[:, :2], q, a, m),                     # frames differ
        lambda: KI.interpolation_l1(pred[:, :, :9], q, a, m),                  # rows differ
        lambda: KI.interpolation_l1(pred[..., :2], q, a, m),                   # fewer than 3 channels
        lambda: training.interpolation_loss([q[0]], a, m, pred),               # one Gaussian set for two samples
        lambda: training.interpolation_loss([q[0], q[1]], a, m, pred[:, :, :9]),
        lambda: training.interpolation_loss([q[0], q[1]], a, m, pred, knn_k=21),
        lambda: KI.knn_interp_weights(q.clone().requires_grad_(True), a),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {i} was accepted")
