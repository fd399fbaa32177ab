"""The rasteriser's call plan (csrc/rast_plan.h), pinned on the host: gvf_rast_call_plan runs the forward's own plan_call, with the forward's
environment switches, and launches nothing.  Every expected value below is written out by hand from the rules:

  bucket = bin_algo != RADIX;  shared = switch & fused & no cov3D_precomp & bucket & P > 0 & F >= 2 & <= 16 slices & F >= 2 n_slices &
  n_slices P 64 <= max_rendered 8;  index_count = bucket & !shared & ntiles <= 4096;  morton = bucket & F >= 4 & P >= 4096;
  slot_mode = shared & switch & morton & SH colours & n_slices P 64 + P M 12 <= max_rendered 8;  rec_gather = bucket & !shared & morton;
  wave_frames = bucket & !shared & switch;  order_tiles = switch & P > 0 & max_rendered > 0 & F ntiles >= 2048.

No second implementation of the rules is called.  No GPU needed."""
import ctypes

import pytest

from gvfdiffusion_amd import _lib
from gvfdiffusion_amd import rasterizer as R

FIELDS = [n for n, _ in _lib.GvfRastPlan._fields_]
MR = 1 << 20          # room for 8 MiB of shared-activation records: ample for every scene here unless a case says otherwise


def frames_of(delta_indices):
    arr = (_lib.GvfRastFrame * len(delta_indices))()
    for f, di in enumerate(delta_indices):
        arr[f].delta_index = di
    return arr


def plan(di, H=256, W=256, P=4096, M=9, max_rendered=MR, bin_algo=_lib.RAST_BIN_AUTO, upstream_binning=False, **kw):
    st = R.make_settings(H, W, 2, _lib.RAST_MODE_MIP, 0.1, 1.0, (0, 0, 0), upstream_binning=upstream_binning, bin_algo=bin_algo)
    p = R.call_plan(st, frames_of(di), P, M, max_rendered, **kw)
    return {n: (list(getattr(p, n)) if n.endswith("_grid") else getattr(p, n)) for n in FIELDS}


# 4 frames of 256 x 256 px (16 x 16 tiles), two delta slices, 4096 Gaussians with 9 SH coefficients: shared activation in slot order.
# LDS: 256 rows x 27 floats x 4 B = 27648 (+16), 64 rows: 6912 (+16).  Clear words: 3 x 1024 + 32768 = 35840 -> 9 blocks of 4096.
BASE = dict(bucket=1, shared=1, index_count=0, morton=1, slot_mode=1, rec_gather=0, wave_frames=0, order_tiles=0, upstream_binning=0,
            n_slices=2, layout=1, gx=16, gy=16, ntiles=256, nb=16, nseg=1024, pre_grid=[16, 1], wf_grid=[64, 1], bin_grid=[4, 4],
            binx_grid=[1, 4], scan_blocks=1, clear_blocks=9, pre_lds_bytes=27664, wf_lds_bytes=6928)
# the same call on the fused path (no shared activation): index-ordered count pass, Morton-ordered gather on the 1-D grid
# ceil(4 / 8) * 8 frames x 4 blocks = 32, wave-frames projection
FUSED = dict(BASE, shared=0, index_count=1, slot_mode=0, layout=0, rec_gather=1, wave_frames=1, bin_grid=[32, 1])


def test_base_case_every_field():
    assert set(BASE) == set(FIELDS)
    assert plan([0, 0, 1, 1]) == BASE


@pytest.mark.parametrize("F, expected", [
    # one frame: never shared, no Morton order (F < 4); clear words 3 x 256 -> 1 block
    (1, dict(FUSED, morton=0, rec_gather=0, n_slices=1, nseg=256, bin_grid=[4, 1], binx_grid=[1, 1], clear_blocks=1)),
    # two and three frames of one slice: shared (F >= 2 x 1), still no Morton order, hence no slot order
    (2, dict(BASE, morton=0, slot_mode=0, layout=0, n_slices=1, nseg=512, bin_grid=[4, 2], binx_grid=[1, 2], clear_blocks=1)),
    (3, dict(BASE, morton=0, slot_mode=0, layout=0, n_slices=1, nseg=768, bin_grid=[4, 3], binx_grid=[1, 3], clear_blocks=1)),
    (4, dict(BASE, n_slices=1)),
])
def test_frame_count_thresholds(F, expected):
    assert plan([0] * F) == expected


@pytest.mark.parametrize("P, expected", [
    # nothing to splat: no shared activation, grids of zero blocks
    (0, dict(FUSED, morton=0, rec_gather=0, n_slices=1, nb=0, pre_grid=[0, 1], wf_grid=[0, 1], bin_grid=[0, 4], binx_grid=[0, 4],
             clear_blocks=1)),
    # one Gaussian short of the Morton order: shared, records at the Gaussians' indices
    (4095, dict(BASE, morton=0, slot_mode=0, layout=0, n_slices=1, clear_blocks=1)),
    (4096, dict(BASE, n_slices=1)),
])
def test_gaussian_count_thresholds(P, expected):
    assert plan([0] * 4, P=P) == expected


def test_index_count_needs_the_tiles_to_fit_its_table():
    # 64 x 64 = 4096 tiles fit, 65 x 64 = 4160 do not; one frame: F ntiles >= 2048 -> heaviest tiles first
    one = dict(FUSED, morton=0, rec_gather=0, order_tiles=1, n_slices=1, bin_grid=[4, 1], binx_grid=[1, 1])
    assert plan([0], H=1024, W=1024) == dict(one, gx=64, gy=64, ntiles=4096, nseg=4096, scan_blocks=1, clear_blocks=3)
    assert plan([0], H=1024, W=1040) == dict(one, index_count=0, gx=65, gy=64, ntiles=4160, nseg=4160, scan_blocks=2, clear_blocks=4)


def test_sixteen_slices_are_shared_seventeen_are_not():
    # 32 frames, 16 slices twice: records 16 x 4096 x 64 = 4 MiB (+ 442368 B of SH rows) <= 8 MiB; 8192 segments
    assert plan(list(range(16)) * 2) == dict(BASE, n_slices=16, order_tiles=1, nseg=8192, pre_grid=[16, 8], wf_grid=[64, 2],
                                             bin_grid=[4, 32], binx_grid=[1, 32], scan_blocks=2, clear_blocks=14)
    # 34 frames, 17 slices: the count stops at 16; fused path, gather grid ceil(34 / 8) x 8 x 4 = 160; 8704 segments
    assert plan(list(range(17)) * 2) == dict(FUSED, n_slices=16, order_tiles=1, nseg=8704, pre_grid=[16, 9], wf_grid=[64, 2],
                                             bin_grid=[160, 1], binx_grid=[1, 34], scan_blocks=3, clear_blocks=15)


def test_two_frames_per_slice_on_average():
    # F = 2 n_slices - 1: not worth it;  F = 2 n_slices: shared (interleaved slices group like ordered ones)
    assert plan([0, 1, 0]) == dict(FUSED, morton=0, rec_gather=0, nseg=768, bin_grid=[4, 3], binx_grid=[1, 3], clear_blocks=1)
    assert plan([0, 1, 0, 1]) == BASE


def test_room_bounds_of_the_records_and_of_the_slot_ordered_sh_copy():
    di = [0, 0, 1, 1]
    # records: 2 x 4096 x 64 B = 524288 = 65536 x 8
    assert plan(di, max_rendered=65535) == FUSED
    assert plan(di, max_rendered=65536) == dict(BASE, slot_mode=0, layout=0)
    # + the SH copy: 4096 x 9 x 3 x 4 = 442368 -> 966656 = 120832 x 8
    assert plan(di, max_rendered=120831) == dict(BASE, slot_mode=0, layout=0)
    assert plan(di, max_rendered=120832) == BASE
    # the sizing call
    assert plan(di, max_rendered=0) == FUSED


def test_blend_order_from_2048_segments():
    one = dict(FUSED, morton=0, rec_gather=0, n_slices=1, bin_grid=[4, 1], binx_grid=[1, 1], clear_blocks=2)
    assert plan([0], H=1424, W=368) == dict(one, gx=23, gy=89, ntiles=2047, nseg=2047)                      # 23 x 89 = 2047
    assert plan([0], H=1024, W=512) == dict(one, order_tiles=1, gx=32, gy=64, ntiles=2048, nseg=2048)       # 32 x 64 = 2048
    assert plan([0], H=1024, W=512, max_rendered=0)["order_tiles"] == 0
    assert plan([0], H=1024, W=512, P=0)["order_tiles"] == 0


def test_input_forms():
    di = [0, 0, 1, 1]
    # precomputed colours: no SH rows in LDS, no slot order
    assert plan(di, has_sh=False, has_colors_precomp=True) == dict(BASE, slot_mode=0, layout=0, pre_lds_bytes=16, wf_lds_bytes=16)
    assert plan(di, has_cov3D_precomp=True) == FUSED
    assert plan(di, fused=False) == FUSED
    # no delta tensor: every frame is slice -1, whatever its index says
    assert plan(di, has_delta=False) == dict(BASE, n_slices=1)
    assert plan([-1, 3, -1, 3]) == BASE
    assert plan(di, has_subpixel_offset=True) == dict(BASE, upstream_binning=1)
    assert plan(di, upstream_binning=True) == dict(BASE, upstream_binning=1)


def test_radix_binning_takes_none_of_the_bucket_paths():
    assert plan([0, 0, 1, 1], bin_algo=_lib.RAST_BIN_RADIX) == dict(BASE, bucket=0, shared=0, morton=0, slot_mode=0, layout=0, clear_blocks=1)
    assert plan([0, 0, 1, 1], bin_algo=_lib.RAST_BIN_BUCKET) == BASE


def test_environment_switches(monkeypatch):
    di = [0, 0, 1, 1]
    monkeypatch.setenv("GVF_RAST_SHARED_ACT", "0")
    assert plan(di) == FUSED
    monkeypatch.setenv("GVF_RAST_PRE_WAVE_FRAMES", "0")
    assert plan(di) == dict(FUSED, wave_frames=0)
    monkeypatch.delenv("GVF_RAST_SHARED_ACT")
    assert plan(di) == BASE                                   # (the wave-frames switch means nothing to a shared call)
    monkeypatch.setenv("GVF_RAST_SLOT_ORDER", "0")
    assert plan(di) == dict(BASE, slot_mode=0, layout=0)
    monkeypatch.setenv("GVF_RAST_SLOT_ORDER", "1")
    assert plan(di) == BASE
    assert plan([0], H=1024, W=512)["order_tiles"] == 1
    monkeypatch.setenv("GVF_RAST_BLEND_ORDER", "0")
    assert plan([0], H=1024, W=512)["order_tiles"] == 0


def test_argument_errors():
    l = _lib.lib()
    st = R.make_settings(256, 256, 2, _lib.RAST_MODE_MIP, 0.1, 1.0, (0, 0, 0))
    fr, out = frames_of([0, 0]), _lib.GvfRastPlan()
    tail = (4096, 9, 1, 1, 0, 0, 1, 0, MR)
    assert l.gvf_rast_call_plan(ctypes.byref(st), fr, 2, *tail, ctypes.byref(out)) == _lib.GVF_OK
    assert l.gvf_rast_call_plan(None, fr, 2, *tail, ctypes.byref(out)) == _lib.GVF_EINVAL
    assert l.gvf_rast_call_plan(ctypes.byref(st), None, 2, *tail, ctypes.byref(out)) == _lib.GVF_EINVAL
    assert l.gvf_rast_call_plan(ctypes.byref(st), fr, 2, *tail, None) == _lib.GVF_EINVAL
    assert l.gvf_rast_call_plan(ctypes.byref(st), fr, 0, *tail, ctypes.byref(out)) == _lib.GVF_EINVAL
    assert l.gvf_rast_call_plan(ctypes.byref(st), fr, -1, *tail, ctypes.byref(out)) == _lib.GVF_EINVAL
    n = ctypes.c_int(0)
    tab = (ctypes.c_int32 * 7)()
    assert l.gvf_rast_slice_groups(None, 2, 1, 0, tab, ctypes.byref(n)) == _lib.GVF_EINVAL
    assert l.gvf_rast_slice_groups(fr, 2, 1, 0, None, ctypes.byref(n)) == _lib.GVF_EINVAL
    assert l.gvf_rast_slice_groups(fr, 2, 1, 0, tab, None) == _lib.GVF_EINVAL
    assert l.gvf_rast_slice_groups(fr, 0, 1, 0, tab, ctypes.byref(n)) == _lib.GVF_EINVAL


def slice_groups(di, has_delta=True, max_slices=0):
    F = len(di)
    tab, n = (ctypes.c_int32 * (3 * F + 1))(), ctypes.c_int(0)
    rc = _lib.lib().gvf_rast_slice_groups(frames_of(di), F, int(has_delta), max_slices, tab, ctypes.byref(n))
    return rc, n.value, list(tab[:F + 2 * n.value + 1])


@pytest.mark.parametrize("di, has_delta, frames, starts, slices", [
    ([0, 0, 1, 1], True, [0, 1, 2, 3], [0, 2, 4], [0, 1]),                         # ordered
    ([2, 0, 2, 0, 1], True, [0, 2, 1, 3, 4], [0, 2, 4, 5], [2, 0, 1]),             # interleaved: slices in order of first use
    ([-1, -1, -1], True, [0, 1, 2], [0, 3], [-1]),                                 # no frame has a delta
    ([5, -1, 5, -7], True, [0, 2, 1, 3], [0, 2, 4], [5, -1]),                      # any negative index is "no delta"
    ([0, 1], False, [0, 1], [0, 2], [-1]),                                         # no delta tensor
    (list(range(17)), True, list(range(17)), list(range(18)), list(range(17))),    # 17 distinct: the backward has no limit
])
def test_slice_grouping_tables(di, has_delta, frames, starts, slices):
    """[F] frames grouped by slice | [n + 1] starts | [n] delta indices: the table the batched backward uploads, and the grouping the
    forward's plan counts."""
    assert slice_groups(di, has_delta) == (_lib.GVF_OK, len(slices), frames + starts + slices)
    assert plan(di, has_delta=has_delta)["n_slices"] == min(len(slices), 16)
    # the forward's limit of 16
    assert slice_groups(di, has_delta, max_slices=16)[0] == (_lib.GVF_ENOSPC if len(slices) > 16 else _lib.GVF_OK)
