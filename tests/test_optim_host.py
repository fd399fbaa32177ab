"""Host side of the fused optimizer step (ops/optim.py, include/gvf_optim.h): the chunk table, the argument checks of the C ABI and
FlatGrads on the CPU, including the in-place all-reduce of training.allreduce_gradients(flat=...) over two gloo ranks.  No GPU."""
import ctypes
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import optim_util as U  # noqa: E402


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_chunk_table_covers_every_element_once_in_order():
    from gvfdiffusion_amd.ops import optim
    C = optim.chunk_len()
    assert C > 0 and C % 4 == 0
    sizes = U.ragged_sizes(C) + [1001]
    table = optim.build_chunk_table(sizes)
    assert table.dtype.itemsize == 16
    expect_tensor, expect_first = 0, 0
    seen = [0] * len(sizes)
    for row in table:
        t, first, count = int(row["tensor"]), int(row["first"]), int(row["count"])
        while sizes[expect_tensor] == expect_first:                      # the previous tensor is complete (or empty): move on
            expect_tensor, expect_first = expect_tensor + 1, 0
        assert t == expect_tensor and first == expect_first, "chunks are not in element order"
        assert 0 < count <= C and first % 4 == 0 and first % C == 0
        assert first + count <= sizes[t], "a chunk crosses its tensor's end"
        seen[t] += count
        expect_first = first + count
    assert seen == sizes
    assert sizes.index(0) not in set(int(t) for t in table["tensor"])
    assert len(table) == sum(math.ceil(n / C) for n in sizes)
    # another chunk length, and the degenerate inputs
    small = optim.build_chunk_table([9, 0, 8, 1], length=4)
    assert [(int(r["tensor"]), int(r["first"]), int(r["count"])) for r in small] == [(0, 0, 4), (0, 4, 4), (0, 8, 1), (2, 0, 4), (2, 4, 4), (3, 0, 1)]
    assert len(optim.build_chunk_table([0, 0])) == 0
    with pytest.raises(ValueError):
        optim.build_chunk_table([4], length=6)
    with pytest.raises(ValueError):
        optim.build_chunk_table([-1])


def _valid_hyper(optim):
    h = optim.GvfOptimHyper()
    h.n_groups, h.n_ema = 2, 2
    h.lr[0], h.lr[1] = 1e-4, 1e-5
    h.weight_decay[0] = 0.01
    h.beta1, h.beta2, h.eps = 0.9, 0.999, 1e-8
    h.ema_rate[0], h.ema_rate[1] = 0.9999, 0.999
    h.max_grad_norm = 1.0
    return h


def test_c_abi_refuses_bad_arguments_without_a_gpu():
    """Every call below is refused by the host-side checks, before any launch; the table pointers are never dereferenced."""
    from gvfdiffusion_amd import _lib
    from gvfdiffusion_amd.ops import optim
    l = _lib.lib()
    EINVAL = _lib.GVF_EINVAL
    out = ctypes.c_size_t(0)
    assert l.gvf_optim_scratch_bytes(100, ctypes.byref(out)) == _lib.GVF_OK and out.value >= 800
    assert l.gvf_optim_scratch_bytes(0, ctypes.byref(out)) == EINVAL
    assert l.gvf_optim_scratch_bytes(-3, ctypes.byref(out)) == EINVAL
    assert l.gvf_optim_scratch_bytes(100, None) == EINVAL
    fake = ctypes.c_void_p(0x10000)      # stands for a device pointer; a refused call never touches it

    def norm(tensors=fake, T=3, chunks=fake, n=100, h=None, record=fake, scratch=fake, nbytes=1 << 20, null_hyper=False):
        h = _valid_hyper(optim) if h is None else h
        return l.gvf_optim_norm(tensors, T, chunks, n, None if null_hyper else ctypes.byref(h), None, record, scratch, nbytes, None)

    def update(tensors=fake, T=3, chunks=fake, n=100, h=None, record=fake, null_hyper=False):
        h = _valid_hyper(optim) if h is None else h
        return l.gvf_optim_adamw_update(tensors, T, chunks, n, None if null_hyper else ctypes.byref(h), None, record, None)

    for call in (norm, update):
        assert call(tensors=None) == EINVAL and call(chunks=None) == EINVAL and call(record=None) == EINVAL
        assert call(null_hyper=True) == EINVAL
        assert call(T=0) == EINVAL and call(T=-1) == EINVAL and call(n=0) == EINVAL and call(n=-5) == EINVAL
        for field, bad in (("n_groups", 9), ("n_groups", 0), ("n_ema", 5), ("n_ema", -1), ("beta1", 1.0), ("beta1", -0.1), ("beta2", 1.0),
                           ("beta2", 1.5), ("beta2", float("nan")), ("eps", 0.0), ("eps", -1e-8), ("max_grad_norm", float("nan"))):
            h = _valid_hyper(optim)
            setattr(h, field, bad)
            assert call(h=h) == EINVAL, (call.__name__, field, bad)
        h = _valid_hyper(optim)
        h.ema_rate[1] = 1.5
        assert call(h=h) == EINVAL
        h = _valid_hyper(optim)
        h.lr[0] = float("inf")
        assert call(h=h) == EINVAL
    assert norm(scratch=None) == EINVAL
    assert norm(nbytes=100 * 8 - 1) == EINVAL          # one double per chunk: too small


def test_fused_adamw_refuses_cpu_and_malformed_parameters():
    from gvfdiffusion_amd import _lib
    from gvfdiffusion_amd.ops.optim import FusedAdamW
    w = torch.nn.Parameter(torch.zeros(8))
    with pytest.raises(_lib.GvfError):
        FusedAdamW([w], lr=1e-3)
    assert w.grad is None                                # refused before anything was attached
    with pytest.raises(ValueError):
        FusedAdamW([torch.nn.Parameter(torch.zeros(8, dtype=torch.float64))], lr=1e-3)
    with pytest.raises(ValueError):
        FusedAdamW([torch.nn.Parameter(torch.zeros(4, 6).t())], lr=1e-3)
    with pytest.raises(ValueError):
        FusedAdamW([w], lr=1e-3, ema_rates=(0.9,) * 5)
    with pytest.raises(ValueError):
        FusedAdamW([w], lr=1e-3, betas=(0.9, 1.0))
    with pytest.raises(ValueError):
        FusedAdamW([w], lr=1e-3, eps=0.0)
    with pytest.raises(ValueError):
        FusedAdamW([{"params": [torch.nn.Parameter(torch.zeros(2))]} for _ in range(9)], lr=1e-3)


def _mlp(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Tanh(), torch.nn.Linear(7, 3))


def test_flat_grads_views_survive_backward_on_cpu():
    from gvfdiffusion_amd.ops.optim import FlatGrads
    net = _mlp()
    frozen = torch.nn.Parameter(torch.ones(3), requires_grad=False)
    params = list(net.parameters()) + [frozen]
    flat = FlatGrads(params)
    assert frozen.grad is None and len(flat.views) == 4
    ptrs = [p.grad.data_ptr() for p in net.parameters()]
    base = flat.buffer.data_ptr()
    assert all((q - base) % 16 == 0 for q in ptrs), "every view starts at a multiple of 4 elements"
    assert flat.buffer.numel() == sum((p.numel() + 3) // 4 * 4 for p in net.parameters())
    x = torch.randn(11, 5)
    net(x).square().sum().backward()
    first = [p.grad.clone() for p in net.parameters()]
    assert [p.grad.data_ptr() for p in net.parameters()] == ptrs and flat.owns(params)
    assert all(float(g.abs().max()) > 0 for g in first)
    net(x).square().sum().backward()                     # accumulates in place
    assert [p.grad.data_ptr() for p in net.parameters()] == ptrs
    for p, g in zip(net.parameters(), first):
        assert torch.allclose(p.grad, 2 * g, rtol=1e-6, atol=0)
    # the buffer and the views are one memory
    off = 0
    for p in net.parameters():
        assert torch.equal(flat.buffer[off:off + p.numel()].view_as(p), p.grad)
        off += (p.numel() + 3) // 4 * 4
    flat.zero_()
    assert all(float(p.grad.abs().max()) == 0 for p in net.parameters()) and flat.owns(params)
    # a dropped or replaced .grad is no longer owned; attach() restores a dropped one
    net[0].weight.grad = None
    assert not flat.owns(params)
    flat.attach()
    assert flat.owns(params) and net[0].weight.grad.data_ptr() == ptrs[0]
    net[0].weight.grad = torch.zeros_like(net[0].weight)
    assert not flat.owns(params)
    # a gradient that exists at construction is kept
    other = _mlp(1)
    other(x).sum().backward()
    kept = [p.grad.clone() for p in other.parameters()]
    flat2 = FlatGrads(other.parameters())
    assert all(torch.equal(p.grad, g) for p, g in zip(other.parameters(), kept)) and flat2.owns(other.parameters())


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gvfdiffusion_amd.ops.optim import FlatGrads
    from gvfdiffusion_amd.training import allreduce_gradients
    net = _mlp()
    params = list(net.parameters())
    flat = FlatGrads(params)
    ptrs = [p.grad.data_ptr() for p in params]
    torch.manual_seed(100 + rank)
    net(torch.randn(9, 5)).square().sum().backward()
    local = [p.grad.clone() for p in params]
    bucket = 64                                            # bytes: several slices
    n_flat = allreduce_gradients(params, bucket_bytes=bucket, flat=flat)
    same = [p.grad.data_ptr() for p in params] == ptrs and flat.owns(params)
    mean_flat = [p.grad.clone() for p in params]
    # the path without `flat` (as before): from the same local gradients, in ordinary .grad tensors
    for p, g in zip(params, local):
        p.grad = g.clone()
    n_plain = allreduce_gradients(params, bucket_bytes=bucket)
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), n_flat=n_flat, n_plain=n_plain, same=same, nbytes=flat.buffer.numel() * 4,
             **{f"local{i}": g.numpy() for i, g in enumerate(local)}, **{f"flat{i}": g.numpy() for i, g in enumerate(mean_flat)},
             **{f"plain{i}": p.grad.numpy() for i, p in enumerate(params)})
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_allreduce_in_place_on_the_flat_buffer(tmp_path):
    world, port = 2, _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r = [np.load(tmp_path / f"r{k}.npz") for k in range(world)]
    for k in range(world):
        assert bool(r[k]["same"]), "the .grad pointers changed"
        assert int(r[k]["n_flat"]) == math.ceil(int(r[k]["nbytes"]) / 64)
        assert int(r[k]["n_plain"]) >= 1
    for i in range(4):
        mean = 0.5 * (r[0][f"local{i}"].astype(np.float64) + r[1][f"local{i}"].astype(np.float64))
        assert np.abs(mean).max() > 0
        for k in range(world):
            assert np.allclose(r[k][f"flat{i}"], mean, rtol=1e-6, atol=1e-30)
            assert np.allclose(r[k][f"plain{i}"], mean, rtol=1e-6, atol=1e-30)
        assert np.array_equal(r[0][f"flat{i}"], r[1][f"flat{i}"])


def test_allreduce_without_a_process_group_is_a_no_op():
    from gvfdiffusion_amd.ops.optim import FlatGrads
    from gvfdiffusion_amd.training import allreduce_gradients
    net = _mlp()
    flat = FlatGrads(net.parameters())
    assert allreduce_gradients(list(net.parameters()), flat=flat) == 0
