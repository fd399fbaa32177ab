"""The rule that picks the bin-record form (csrc/rast_plan.h, plan_call), through the diagnostic entry gvf_rast_bin_record_bytes, which runs
the forward's own plan_call with the forward's environment switches:

  8 bytes  iff  bucket binning  &  gx <= 255  &  gy <= 255  &  GVF_RAST_BIN_REC8 is not "0";  else 16.

gx = ceil(W / 16), gy = ceil(H / 16): 4080 px are 255 tiles, 4081 px are 256.  No GPU needed."""
import ctypes

import pytest

from gvfdiffusion_amd import _lib
from gvfdiffusion_amd import rasterizer as R


def rec_bytes(H, W, bin_algo=_lib.RAST_BIN_AUTO):
    return R.bin_record_bytes(R.make_settings(H, W, 2, _lib.RAST_MODE_MIP, 0.1, 1.0, (0, 0, 0), bin_algo=bin_algo))


@pytest.fixture(autouse=True)
def switch_unset(monkeypatch):
    monkeypatch.delenv("GVF_RAST_BIN_REC8", raising=False)


@pytest.mark.parametrize("H, W, expected", [
    (800, 800, 8),                                    # the bench shape: 50 x 50 tiles
    (16, 16, 8),
    (32, 4080, 8), (32, 4081, 16), (32, 4096, 16),    # 255 | 256 tile columns
    (4080, 32, 8), (4081, 32, 16), (4096, 32, 16),    # 255 | 256 tile rows
    (4080, 4080, 8), (4080, 4096, 16), (4096, 4080, 16),
])
def test_grid_threshold_on_either_axis(H, W, expected):
    assert rec_bytes(H, W) == expected


def test_radix_binning_keeps_no_8_byte_records():
    assert rec_bytes(800, 800, _lib.RAST_BIN_RADIX) == 16
    assert rec_bytes(800, 800, _lib.RAST_BIN_BUCKET) == 8


def test_switch_is_read_per_call(monkeypatch):
    assert rec_bytes(800, 800) == 8
    monkeypatch.setenv("GVF_RAST_BIN_REC8", "0")
    assert rec_bytes(800, 800) == 16 and rec_bytes(32, 4096) == 16
    monkeypatch.setenv("GVF_RAST_BIN_REC8", "1")
    assert rec_bytes(800, 800) == 8 and rec_bytes(32, 4096) == 16       # the switch cannot force 8 bytes onto a grid that does not fit
    monkeypatch.delenv("GVF_RAST_BIN_REC8")
    assert rec_bytes(800, 800) == 8


def test_the_public_plan_and_the_workspace_do_not_depend_on_the_form(monkeypatch):
    frames = (_lib.GvfRastFrame * 8)()

    def public():
        p = R.call_plan(R.make_settings(800, 800, 2, _lib.RAST_MODE_MIP, 0.1, 1.0, (0, 0, 0)), frames, 40_000, 9, 1 << 20)
        return bytes(p), R.workspace_bytes(40_000, 8, 800, 800, 1 << 20)
    on = public()
    monkeypatch.setenv("GVF_RAST_BIN_REC8", "0")
    assert public() == on


def test_argument_errors():
    l = _lib.lib()
    st = R.make_settings(256, 256, 2, _lib.RAST_MODE_MIP, 0.1, 1.0, (0, 0, 0))
    out = ctypes.c_int(0)
    assert l.gvf_rast_bin_record_bytes(ctypes.byref(st), ctypes.byref(out)) == _lib.GVF_OK and out.value == 8
    assert l.gvf_rast_bin_record_bytes(None, ctypes.byref(out)) == _lib.GVF_EINVAL
    assert l.gvf_rast_bin_record_bytes(ctypes.byref(st), None) == _lib.GVF_EINVAL
    st.image_width = 0
    assert l.gvf_rast_bin_record_bytes(ctypes.byref(st), ctypes.byref(out)) == _lib.GVF_EINVAL
