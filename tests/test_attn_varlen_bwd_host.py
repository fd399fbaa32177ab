"""Host side of the ragged attention backward (gvf_attn_varlen_bwd, ops/attention_grad.py::attention_varlen, the enable_training switch of
SparseMultiHeadAttention): the entry points exist, every argument error is refused before any launch, the workspace is large enough, and
the packed float64 reference of tests/attn_varlen_ref.py agrees with one dense block-diagonal computation.  No GPU is needed."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import attn_bwd_ref as R
import attn_varlen_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELF_LENS = [1, 31, 32, 33, 127, 128, 129, 218, 260]
CROSS_Q = [40, 0, 130, 5, 1024]
CROSS_K = [300, 64, 0, 33, 64]


def _lib():
    from gvfdiffusion_amd import _lib
    from gvfdiffusion_amd.ops import attention_grad  # noqa: F401  (registers the signatures)
    return _lib


def test_header_declares_and_library_exports_both_entry_points():
    src = open(os.path.join(ROOT, "include", "gvf_attn_bwd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = _lib()
    for name in ("gvf_attn_varlen_bwd_workspace_bytes", "gvf_attn_varlen_bwd"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), f"{name} is not declared in include/gvf_attn_bwd.h"
        assert name in L.SIGNATURES
        assert hasattr(L.lib(), name)


def _ws(n_seqs=5, tq=1199, tk=461, mq=1024, mk=300, H=2, D=64):
    nb = ctypes.c_size_t(0)
    rc = _lib().lib().gvf_attn_varlen_bwd_workspace_bytes(n_seqs, tq, tk, mq, mk, H, D, ctypes.byref(nb))
    return rc, nb.value


def test_workspace_size():
    L = _lib()
    rc, base = _ws()
    assert rc == 0
    # lse2 and delta, fp32 [H][total_q] each; this shape (3 key blocks x 10 problems against 32 query tiles) splits the key sweep
    assert base >= 2 * 4 * 2 * 1199 + 2 * 2 * 4 * 2 * 461 * 64
    assert _ws(H=40)[1] < 2 * 4 * 40 * 1199 + 4096, "300 key-sweep workgroups need no split"
    for H in (1, 2, 12):
        for D in (32, 64):
            for tq in (0, 1, 1199, 20000):
                assert _ws(tq=tq, H=H, D=D)[1] >= 2 * 4 * H * tq
    # monotone in the totals with everything else fixed, split or not; without a split (short queries) in H as well
    for kw in ({}, {"mq": 218, "mk": 218}):
        sizes = [_ws(tq=t, **kw)[1] for t in (0, 1, 100, 1199, 50000)]
        assert sizes == sorted(sizes)
        sizes = [_ws(tk=t, **kw)[1] for t in (0, 1, 100, 461, 50000)]
        assert sizes == sorted(sizes)
    sizes = [_ws(H=h, mq=218, mk=218)[1] for h in (1, 2, 3, 12, 64)]
    assert sizes == sorted(sizes)
    assert _ws(mq=218, mk=218, n_seqs=5)[1] == _ws(mq=218, mk=218, n_seqs=500)[1]
    E = L.GVF_EINVAL
    for bad in ({"n_seqs": 0}, {"n_seqs": -1}, {"H": 0}, {"mq": 0}, {"mk": 0}, {"mk": -3}, {"tq": -1}, {"tk": -1}, {"D": 48}, {"D": 128},
                {"tq": 2 ** 31}, {"tk": 2 ** 31}):
        assert _ws(**bad)[0] == E, bad
    assert L.lib().gvf_attn_varlen_bwd_workspace_bytes(5, 10, 10, 4, 4, 2, 64, None) == E


def test_every_argument_error_is_refused_on_the_host():
    """GVF_EINVAL before any launch: the pointers are host memory that is never dereferenced (there is no device here)."""
    L = _lib()
    l, E = L.lib(), L.GVF_EINVAL
    i64x4 = ctypes.c_int64 * 4
    raw = ctypes.create_string_buffer(4096 + 64)
    base = (ctypes.addressof(raw) + 63) // 64 * 64           # 64-byte aligned stand-ins for device addresses
    ok_s = i64x4(0, 0, 128, 64)
    rc, need = _ws()
    assert rc == 0

    def call(**kw):
        a = dict(dtype=0, q=base, k=base + 64, v=base + 128, o=base + 192, do=base + 256, dq=base + 320, dk=base + 384, dv=base + 448,
                 n_seqs=5, cu_q=base + 512, cu_k=base + 576, tq=1199, tk=461, mq=1024, mk=300, H=2, D=64,
                 s=[ok_s] * 8, scale=0.125, ws=base + 1024, ws_bytes=need)
        a.update(kw)
        s = a["s"]
        return l.gvf_attn_varlen_bwd(a["dtype"], a["q"], a["k"], a["v"], a["o"], a["do"], a["dq"], a["dk"], a["dv"], a["n_seqs"], a["cu_q"],
                                     a["cu_k"], a["tq"], a["tk"], a["mq"], a["mk"], a["H"], a["D"], s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7],
                                     a["scale"], a["ws"], a["ws_bytes"], None)

    for name in ("q", "k", "v", "o", "do", "dq", "dk", "dv", "cu_q", "cu_k", "ws"):
        assert call(**{name: None}) == E, f"null {name}"
    for i in range(8):
        s = [ok_s] * 8
        s[i] = None
        assert call(s=s) == E, f"null stride array {i}"
    for bad in ({"dtype": 2}, {"dtype": -1}, {"D": 16}, {"D": 128}, {"n_seqs": 0}, {"n_seqs": -2}, {"H": 0}, {"H": -1}, {"mq": 0}, {"mk": 0},
                {"mq": -7}, {"tq": -1}, {"tk": -1}, {"scale": 0.0}, {"scale": -1.0}, {"scale": float("nan")}, {"scale": float("inf")},
                {"ws_bytes": need - 1}, {"ws_bytes": 0}, {"ws": base + 1024 + 8}):
        assert call(**bad) == E, bad
    for name in ("q", "k", "v", "o", "do"):                   # inputs: 16-byte bases, strides multiples of 8 elements
        assert call(**{name: base + 8}) == E, f"{name} 8-byte aligned only"
    for name in ("dq", "dk", "dv"):                            # gradients: 8-byte bases, strides multiples of 4 elements
        assert call(**{name: base + 320 + 4}) == E, f"{name} 4-byte aligned only"
    for i in range(8):
        for j in (0, 2, 3):
            st = list(ok_s)
            st[j] += 4 if i < 5 else 2
            s = [ok_s] * 8
            s[i] = i64x4(*st)
            assert call(s=s) == E, (i, j)


def test_operator_refuses_cpu_tensors_and_misfits():
    L = _lib()
    from gvfdiffusion_amd.ops import attention_grad as AG
    q, k, v, do = V.make_packed([3, 4], [5, 2], 2, 32, torch.float16)
    cq, ck = V.cu([3, 4]), V.cu([5, 2])
    with pytest.raises(L.GvfError):
        AG.attention_varlen(q, k, v, cq, ck, 4, 5)
    with pytest.raises(L.GvfError):
        AG.attention_varlen_backward(q, k, v, q, do, cq, ck, 4, 5, 0.2)
    with pytest.raises(ValueError):
        AG.attention_varlen(q[None], k, v, cq, ck, 4, 5)
    assert callable(AG.varlen_workspace_bytes) and AG.varlen_workspace_bytes(2, 7, 7, 4, 5, 2, 32) >= 2 * 4 * 2 * 7


def test_enable_training_toggles_and_leaves_the_inference_path_alone():
    from gvfdiffusion_amd.sparse.attention.modules import SparseMultiHeadAttention
    m = SparseMultiHeadAttention(64, 2, qk_rms_norm=True)
    assert m.train_forward is False
    keys = set(m.state_dict())
    assert m.enable_training() is m and m.train_forward is True and m.train_dtype is None
    assert m.enable_training(dtype=torch.float16).train_dtype == torch.float16
    assert m.enable_training(False).train_forward is False
    with pytest.raises(ValueError):
        m.enable_training(dtype=torch.float32)
    assert set(m.state_dict()) == keys, "the switch adds nothing to the state dict"
    # off (and under no_grad): forward never reaches the training route
    called = []
    m._forward_train = lambda *a, **k: called.append(1)
    src = inspect.getsource(SparseMultiHeadAttention.forward)
    assert "self.train_forward and torch.is_grad_enabled()" in src
    m.enable_training()
    with torch.no_grad(), pytest.raises(Exception):          # the inference route: CPU tensors are refused by its first kernel
        m(torch.zeros(1, 4, 64))
    m.enable_training(False)
    with pytest.raises(Exception):
        m(torch.zeros(1, 4, 64))
    assert not called


@pytest.mark.parametrize("q_lens,k_lens", [(SELF_LENS, SELF_LENS), (CROSS_Q, CROSS_K)], ids=["self", "cross"])
def test_packed_reference_against_one_block_diagonal_computation(q_lens, k_lens):
    H, C = 2, 32
    q, k, v, do = V.make_packed(q_lens, k_lens, H, C, torch.float16, seed=5)
    scale = C ** -0.5
    looped = V.packed_grads64(q, k, v, do, q_lens, k_lens, scale)
    dense = V.block_diagonal_grads64(q, k, v, do, q_lens, k_lens, scale)
    for name, a, b in zip(("o", "dq", "dk", "dv"), looped, dense):
        assert a.shape == b.shape and a.dtype == torch.float64
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), name
    # the empty-key sequence has zero output and dq rows, the empty-query sequence zero dk and dv rows, in both
    for (a, b), (c, d) in zip(V.bounds(q_lens), V.bounds(k_lens)):
        if d == c:
            assert not looped[0][a:b].any() and not looped[1][a:b].any() and not dense[1][a:b].any()
        if b == a:
            assert not looped[2][c:d].any() and not looped[3][c:d].any() and not dense[3][c:d].any()


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["float16", "bfloat16"])
@pytest.mark.parametrize("C", [32, 64])
def test_gpu_test_inputs_have_no_zero_reference_norm(C, dt):
    """The per-sequence relative measures of tests/test_attn_varlen_bwd_gpu.py need a non-zero reference norm in every non-empty sequence.
    The one exception is exact: with ONE key p = 1 and dP - delta = 0, so dQ and dK of the length-1 sequence are zero in exact arithmetic;
    the GPU test holds them element by element to the floor of tests/test_attn_bwd_gpu.py instead.  The yardstick stays within its own
    2x bar by construction."""
    for q_lens, k_lens, seed in ((SELF_LENS, SELF_LENS, 21), (CROSS_Q, CROSS_K, 22)):
        q, k, v, do = V.make_packed(q_lens, k_lens, 2, C, dt, seed=seed)
        ref = V.packed_grads64(q, k, v, do, q_lens, k_lens, C ** -0.5)
        for (a, b), (c, d) in zip(V.bounds(q_lens), V.bounds(k_lens)):
            if b == a or d == c:
                continue
            one_key = d - c == 1
            assert (float(ref[1][a:b].norm()) > 0) != one_key and (float(ref[2][c:d].norm()) > 0) != one_key
            assert float(ref[3][c:d].norm()) > 0
