"""The helpers the operator modules share (gvfdiffusion_amd/ops/_util.py): which 2-D views the row kernels read in place and which are
copied first, and the size query in front of a scratch allocation.  CPU tensors, no GPU."""
import pytest
import torch

from gvfdiffusion_amd import _lib
from gvfdiffusion_amd.ops import _util
from gvfdiffusion_amd.ops import sparse_train  # noqa: F401  (registers gvf_colsum_f32_workspace_bytes)


def _bf16(rows, cols):
    return torch.arange(rows * cols, dtype=torch.float32).reshape(rows, cols).to(torch.bfloat16)


def _in_place(x):
    y = _util.rows16(x)
    return y.data_ptr() == x.data_ptr() and y.stride() == x.stride()


def _copied(x):
    y = _util.rows16(x)
    return y.data_ptr() != x.data_ptr() and y.is_contiguous() and torch.equal(y, x)


def test_rows16_reads_16_byte_rows_in_place():
    wide = _bf16(5, 40)
    assert wide.data_ptr() % 16 == 0
    assert _in_place(_bf16(5, 16))
    assert _in_place(wide[:, 8:24])                                                     # row stride 80 bytes, base 16 bytes in
    assert _in_place(torch.empty(64, dtype=torch.bfloat16).as_strided((1, 16), (17, 1)))   # one row: its nominal stride is never used


def test_rows16_copies_what_16_byte_loads_cannot_address():
    wide = _bf16(5, 40)
    assert _copied(wide[:, 4:20])                                                       # base 8 bytes off
    assert _copied(_bf16(5, 36)[:, :16])                                                # row stride 72 bytes
    assert _copied(_bf16(16, 5).t())                                                    # no unit column stride
    assert _copied(torch.arange(18, dtype=torch.float32).reshape(3, 6)[:, 1:5])         # fp32: row stride 24 bytes, base 4 bytes off


def test_workspace_bytes_is_the_checked_size_query():
    nb = _util.workspace_bytes("gvf_colsum_f32_workspace_bytes", 64, 32)
    assert type(nb) is int and nb > 0
    with pytest.raises(_lib.GvfError):
        _util.workspace_bytes("gvf_colsum_f32_workspace_bytes", -1, 32)
