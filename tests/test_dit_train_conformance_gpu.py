"""The training kernels of csrc/dit_train.hip held element by element to the float64 reference and the derived bounds of
tests/dit_train_bounds.py (checked on the CPU by tests/test_dit_train_conformance_ref.py), both 16-bit types, over every dispatch path:
VPL = 1 .. 4 and the generic kernels, NCH = 1, 2 and 4 (H d = 1280 runs the NCH = 4 instantiation with an empty trip), the second trip of the
forward's base loop, groups cut inside workgroups, a group over 129 slots (the finaliser's w += 4 loop), more than 1024 groups (its grid wrap),
rows_per_group = 1 and rows_per_group > rows.  No element is exempt but the dx of the one planted all-zero RMSNorm row (u / 1e-12), which
keeps the exact-value check of tests/test_dit_train_ops_gpu.py; guard rows, NaN padding of the outputs, relaunch and other-stream checks
live there and are not repeated.  The workspace is NaN-filled: a finaliser that reads a slot nobody wrote shows as NaN.
pytest -s prints the largest |err| / bound of every output."""
import functools

import pytest
import torch

import dit_train_bounds as B
import dit_train_ref as R
from gvfdiffusion_amd import _lib
from gvfdiffusion_amd.ops import dit_ops
from test_dit_train_ops_gpu import _guarded, _ws, _p, _stream_ptr

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "fp16"]


def _ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


def _path(C):
    return f"VPL{C // 256}" if B.vec_path(C) else "generic"


def _hold(tag, name, got, model, log, dt=None, keep=None):
    """no element of `got` outside the bound of model = (ref, bound) | (ref, E, bound of the 16-bit store)"""
    ref = model[0]
    got = got.cpu().reshape(ref.shape)
    if keep is not None:
        got, model = got[keep], tuple(t[keep] for t in model)
    if len(model) == 3:
        n_bad, worst = B.check16(got, model[0], model[1], dt)
    else:
        n_bad, worst = B.excess(got, model[0], model[1])
    log.append(f"{name} {worst:.3f}")
    assert n_bad == 0, f"{tag} {name}: {n_bad} of {got.numel()} elements outside the bound (worst |err| / bound {worst:.3g})"


@functools.lru_cache(maxsize=4)
def _ln_inputs(case, dt):
    return B.make_ln(*case, dt)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mode", B.MODES)
@pytest.mark.parametrize("case", B.LN_CASES, ids=_ids(B.LN_CASES))
def test_layernorm_modulate_backward_elementwise(cuda, case, mode, dt):
    C, rows, rpg = case
    d = _ln_inputs(case, dt)
    G, ld = d["G"], d["ld"]
    has_mod, has_aff = mode in ("adaln", "both"), mode in ("affine", "both")
    dev = cuda
    xd, dyd, md, dresd = d["x"].to(dev), d["dy"].to(dev), d["mod"].to(dev), d["dres"].to(dev)
    wd, bd = (d["w"].to(dev), d["b"].to(dev)) if has_aff else (None, None)
    scd = md[:, d["scale_off"]:] if has_mod else None
    code = dit_ops.dt_code(dt)
    sp = _stream_ptr(torch.cuda.current_stream())
    for with_dres in (True, False):
        model = B.ln_bwd(d["x"], d["dy"], **B.ln_args(d, mode, with_dres))
        _, dx = _guarded(rows, C, torch.float32, dev)
        _, dsh = _guarded(G, C, torch.float32, dev)
        _, dsc = _guarded(G, C, torch.float32, dev)
        _, dw = _guarded(1, C, torch.float32, dev)
        _, db = _guarded(1, C, torch.float32, dev)
        ws = _ws("gvf_ln_mod_bwd_workspace_bytes", dev, rows, C, rpg if has_mod else 0)
        _lib.check(_lib.lib().gvf_ln_mod_bwd(code, _p(xd), _p(dyd), _p(dresd) if with_dres else None, _p(dx), rows, C, 1e-6, _p(wd), _p(bd), _p(scd), ld, rpg,
                                             _p(dsh) if has_mod else None, _p(dsc) if has_mod else None, _p(dw) if has_aff else None,
                                             _p(db) if has_aff else None, _p(ws), ws.numel() * 4, sp), "bwd")
        torch.cuda.synchronize()
        tag, log = f"ln_bwd {_path(C)} C{C} rows{rows} rpg{rpg} {mode} {'dres' if with_dres else 'nodres'} {DT_IDS[DTYPES.index(dt)]}", []
        got = dict(dx=dx, dshift=dsh, dscale=dsc, dw=dw, db=db)
        for name, mb in model.items():
            _hold(tag, name, got[name], mb, log)
        print("RATIO", tag, "|", "; ".join(log))


@functools.lru_cache(maxsize=4)
def _gate_inputs(case, dt):
    return B.make_gate(*case, dt)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("gated", [True, False], ids=["gate", "nogate"])
@pytest.mark.parametrize("case", B.LN_CASES, ids=_ids(B.LN_CASES))
def test_gate_residual_elementwise(cuda, case, gated, dt):
    C, rows, rpg = case
    d = _gate_inputs(case, dt)
    G, ld = d["G"], d["ld"]
    model = B.gate_fwd_bwd(d["x"], d["h"], d["dout"], d["gate"] if gated else None, rpg, dt)
    dev = cuda
    xd, hd, dd, td = d["x"].to(dev), d["h"].to(dev), d["dout"].to(dev), d["tab"].to(dev)
    gd = td[:, 4:] if gated else None
    _, out = _guarded(rows, C, torch.float32, dev)
    _, dh = _guarded(rows, C, dt, dev)
    _, dgate = _guarded(G, C, torch.float32, dev)
    ws = _ws("gvf_gate_residual_bwd_workspace_bytes", dev, rows, C, rpg if gated else 0)
    code = dit_ops.dt_code(dt)
    sp = _stream_ptr(torch.cuda.current_stream())
    _lib.check(_lib.lib().gvf_gate_residual_fwd(code, _p(xd), _p(hd), _p(gd), ld, rpg, _p(out), rows, C, sp), "fwd")
    _lib.check(_lib.lib().gvf_gate_residual_bwd(code, _p(dd), _p(hd) if gated else None, _p(gd), ld, rpg, _p(dh), _p(dgate) if gated else None, rows, C,
                                                _p(ws) if gated else None, ws.numel() * 4 if gated else 0, sp), "bwd")
    torch.cuda.synchronize()
    tag, log = f"gate {_path(C)} C{C} rows{rows} rpg{rpg} {'gate' if gated else 'nogate'} {DT_IDS[DTYPES.index(dt)]}", []
    _hold(tag, "out", out, model["out"], log)
    ref, bnd = model["dh"]
    n_bad, worst = B.excess(dh.cpu(), ref, bnd)
    log.append(f"dh {worst:.3f}")
    assert n_bad == 0, f"{tag} dh: {n_bad} elements outside their interval (worst {worst:.3g})"
    if gated:
        _hold(tag, "dgate", dgate, model["dgate"], log)
    print("RATIO", tag, "|", "; ".join(log))


def _rms_once(cuda, tag, d, dt, xv, ldx):
    rows, H, dd = d["rows"], d["H"], d["d"]
    HD = H * dd
    model = B.rms_fwd_bwd(d["x"], d["dy"], d["gamma"], dt)
    dev = cuda
    gd, dyd = d["gamma"].to(dev), d["dy"].reshape(rows, HD).to(dev)
    _, y = _guarded(rows, HD, dt, dev)
    _, dx = _guarded(rows, HD, dt, dev)
    _, dgamma = _guarded(1, HD, torch.float32, dev)
    ws = _ws("gvf_rmsnorm_heads_bwd_workspace_bytes", dev, rows, H, dd)
    code = dit_ops.dt_code(dt)
    sp = _stream_ptr(torch.cuda.current_stream())
    _lib.check(_lib.lib().gvf_rmsnorm_heads_fwd(code, _p(xv), ldx, _p(gd), _p(y), HD, rows, H, dd, sp), "fwd")
    _lib.check(_lib.lib().gvf_rmsnorm_heads_bwd(code, _p(xv), ldx, _p(dyd), HD, _p(gd), _p(dx), HD, _p(dgamma), rows, H, dd, _p(ws), ws.numel() * 4, sp), "bwd")
    torch.cuda.synchronize()
    log = []
    zero_row = d["zero_row"]
    got_dx = dx.cpu().reshape(rows, H, dd)
    # the planted all-zero row: u / 1e-12 leaves the 16-bit range in fp16 (inf) and stays finite in bf16 -- exactly the rounded float64 value
    want = model["dx"][0][zero_row].to(dt)
    assert torch.equal(got_dx[zero_row].view(torch.int16), want.view(torch.int16)) or R.rel_l2(got_dx[zero_row], want) <= 2 ** -7, f"{tag}: the all-zero row"
    assert float(got_dx[zero_row].float().abs().max()) > 1e9
    keep = torch.ones(rows, dtype=torch.bool)
    keep[zero_row] = False
    _hold(tag, "y", y, model["y"], log, dt)
    _hold(tag, "dx", dx, model["dx"], log, dt, keep)
    _hold(tag, "dgamma", dgamma, model["dgamma"], log)
    print("RATIO", tag, "|", "; ".join(log))


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", B.RMS_CASES, ids=_ids(B.RMS_CASES))
def test_rmsnorm_heads_elementwise(cuda, case, dt):
    rows, H, dd = case
    d = B.make_rms(rows, H, dd, dt)
    nch = (H * dd + 511) // 512
    _rms_once(cuda, f"rms NCH{nch} rows{rows} H{H} d{dd} contiguous {DT_IDS[DTYPES.index(dt)]}", d, dt, d["x"].reshape(rows, H * dd).to(cuda), H * dd)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", B.RMS_PACKED, ids=_ids(B.RMS_PACKED))
def test_rmsnorm_heads_elementwise_packed_qkv(cuda, case, dt):
    """q and k read in place from a packed [q | k | v] projection whose v slice is NaN"""
    rows, H, dd = case
    HD = H * dd
    slices = [B.make_rms(rows, H, dd, dt, seed=1), B.make_rms(rows, H, dd, dt, seed=2, scale=0.5)]
    qkv = torch.full((rows, 3 * HD), float("nan"), dtype=dt, device=cuda)
    for i, d in enumerate(slices):
        qkv[:, i * HD:(i + 1) * HD] = d["x"].reshape(rows, HD).to(cuda)
    nch = (HD + 511) // 512
    for i, d in enumerate(slices):
        _rms_once(cuda, f"rms NCH{nch} rows{rows} H{H} d{dd} packed[{i}] {DT_IDS[DTYPES.index(dt)]}", d, dt, qkv[:, i * HD:(i + 1) * HD], 3 * HD)
    assert bool(torch.isnan(qkv[:, 2 * HD:].float()).all()), "the v slice of the packed buffer was written"
