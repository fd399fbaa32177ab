"""CPU oracle -- TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this package
(never gvfdiffusion_amd/).  It wraps the plain-C restatements in this directory
(rast_oracle.c, rast_bwd_oracle.c, vox2seq_oracle.c -> libgvf_oracle.so; rast_bwd_oracle.c in single precision ->
libgvf_oracle_f32.so, the fp32 yardstick; both built by `make -C oracle`) and holds the
torch-fp32 restatements of the floating-point DiT / sampler path (dit_ref.py, dpm_ref.py).
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
_LIB32 = None


def build(force: bool = False) -> str:
    so = os.path.join(_HERE, "libgvf_oracle.so")
    sos = (so, os.path.join(_HERE, "libgvf_oracle_f32.so"))
    srcs = [os.path.join(_HERE, f) for f in ("rast_oracle.c", "rast_bwd_oracle.c", "vox2seq_oracle.c", "Makefile")]
    stale = any((not os.path.exists(o)) or any(os.path.getmtime(s) > os.path.getmtime(o) for s in srcs) for o in sos)
    if force or stale:
        subprocess.check_call(["make", "-C", _HERE, "-B", "all"], stdout=subprocess.DEVNULL)
    return so


def lib():
    global _LIB
    if _LIB is None:
        _LIB = ctypes.CDLL(build())
    return _LIB


def lib32():
    """The fp32 yardstick of the rasteriser backward (gvfo32_*)."""
    global _LIB32
    if _LIB32 is None:
        build()
        _LIB32 = ctypes.CDLL(os.path.join(_HERE, "libgvf_oracle_f32.so"))
    return _LIB32


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a, ty=ctypes.c_float):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ty))


def num_threads() -> int:
    return int(lib().gvfo_num_threads())


def _common(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp):
    means3D = _f32(means3D)
    P = means3D.shape[0]
    shs = _f32(shs)
    M = 0 if shs is None else shs.shape[1]
    return (P, M, means3D, shs, _f32(colors_precomp), _f32(np.reshape(opacities, (-1,))), _f32(scales),
            _f32(rotations), _f32(cov3D_precomp))


def rast_preprocess(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, *, H, W,
                    tanfovx, tanfovy, kernel_size, scale_modifier, mode, viewmatrix, projmatrix, campos,
                    sh_degree, tight=False):
    lib().gvfo_set_tight_binning(int(bool(tight)))
    P, M, m3, sh, cp, op, sc, ro, c3 = _common(means3D, shs, colors_precomp, opacities, scales, rotations,
                                               cov3D_precomp)
    geom = np.zeros((P, 24), np.float32)
    v, pj, cam = _f32(np.reshape(viewmatrix, (-1,))), _f32(np.reshape(projmatrix, (-1,))), _f32(campos)
    rc = lib().gvfo_preprocess(P, M, int(sh_degree), _ptr(m3), _ptr(sh), _ptr(cp), _ptr(op), _ptr(sc), _ptr(ro),
                               _ptr(c3), int(H), int(W), ctypes.c_float(tanfovx), ctypes.c_float(tanfovy),
                               ctypes.c_float(kernel_size), ctypes.c_float(scale_modifier), int(mode), _ptr(v),
                               _ptr(pj), _ptr(cam), _ptr(geom))
    lib().gvfo_set_tight_binning(0)
    assert rc == 0
    return geom


def rast_render(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, *, H, W, tanfovx,
                tanfovy, kernel_size, scale_modifier, mode, viewmatrix, projmatrix, campos, sh_degree, bg,
                subpixel_offset=None, nthreads=0, brute=False, tight=False):
    """Returns dict(color[3,H,W], alpha[H,W], depth[H,W], radii[P], num_rendered, flags[H,W]).
    tight=True: drop (Gaussian, tile) instances that cannot reach alpha 1/255 anywhere in the tile (the HIP
    path's default binning; same image, smaller num_rendered) instead of upstream's 3-sigma rect."""
    lib().gvfo_set_tight_binning(int(bool(tight)))
    P, M, m3, sh, cp, op, sc, ro, c3 = _common(means3D, shs, colors_precomp, opacities, scales, rotations,
                                               cov3D_precomp)
    v, pj, cam = _f32(np.reshape(viewmatrix, (-1,))), _f32(np.reshape(projmatrix, (-1,))), _f32(campos)
    bg = _f32(bg)
    color = np.zeros((3, H, W), np.float32)
    alpha = np.zeros((H, W), np.float32)
    depth = np.zeros((H, W), np.float32)
    radii = np.zeros((P,), np.int32)
    nr = np.zeros((1,), np.uint32)
    flags = np.zeros((H, W), np.uint8)
    f = ctypes.c_float
    if brute:
        rc = lib().gvfo_render_brute(P, M, int(sh_degree), _ptr(m3), _ptr(sh), _ptr(cp), _ptr(op), _ptr(sc),
                                     _ptr(ro), _ptr(c3), int(H), int(W), f(tanfovx), f(tanfovy), f(kernel_size),
                                     f(scale_modifier), int(mode), _ptr(v), _ptr(pj), _ptr(cam), _ptr(bg),
                                     _ptr(color), _ptr(alpha), _ptr(depth))
    else:
        so = _f32(subpixel_offset)
        rc = lib().gvfo_render(P, M, int(sh_degree), _ptr(m3), _ptr(sh), _ptr(cp), _ptr(op), _ptr(sc), _ptr(ro),
                               _ptr(c3), _ptr(so), int(H), int(W), f(tanfovx), f(tanfovy), f(kernel_size),
                               f(scale_modifier), int(mode), _ptr(v), _ptr(pj), _ptr(cam), _ptr(bg), _ptr(color),
                               _ptr(alpha), _ptr(depth), _ptr(radii, ctypes.c_int32), _ptr(nr, ctypes.c_uint32),
                               _ptr(flags, ctypes.c_uint8), int(nthreads))
    lib().gvfo_set_tight_binning(0)
    assert rc == 0, rc
    return dict(color=color, alpha=alpha, depth=depth, radii=radii, num_rendered=int(nr[0]), flags=flags)


def gaussian_activate(xyz_raw, features_dc, scaling_raw, rotation_raw, opacity_raw, delta, *, aabb, scale_bias,
                      opacity_bias, min_kernel_size, scaling_activation):
    xyz_raw = _f32(xyz_raw); P = xyz_raw.shape[0]
    features_dc = _f32(features_dc); M = features_dc.shape[1]
    scaling_raw, rotation_raw = _f32(scaling_raw), _f32(rotation_raw)
    opacity_raw = _f32(np.reshape(opacity_raw, (-1,)))
    delta = _f32(delta)
    aabb = _f32(aabb)
    out = dict(means3D=np.zeros((P, 3), np.float32), scales=np.zeros((P, 3), np.float32),
               rotations=np.zeros((P, 4), np.float32), shs=np.zeros((P, M, 3), np.float32),
               opacities=np.zeros((P,), np.float32))
    f = ctypes.c_float
    rc = lib().gvfo_activate(P, M, _ptr(aabb), f(scale_bias), f(opacity_bias), f(min_kernel_size),
                             int(scaling_activation), _ptr(xyz_raw), _ptr(features_dc), _ptr(scaling_raw),
                             _ptr(rotation_raw), _ptr(opacity_raw), _ptr(delta), _ptr(out["means3D"]),
                             _ptr(out["scales"]), _ptr(out["rotations"]), _ptr(out["shs"]), _ptr(out["opacities"]))
    assert rc == 0
    return out


def _vox(fn, a, b, c, n_out):
    a = np.ascontiguousarray(a, np.int32); n = a.shape[0]
    ip = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    if n_out == 1:
        b = np.ascontiguousarray(b, np.int32); c = np.ascontiguousarray(c, np.int32)
        out = np.zeros((n,), np.int32)
        fn(ctypes.c_int64(n), ip(a), ip(b), ip(c), ip(out))
        return out
    x, y, z = (np.zeros((n,), np.int32) for _ in range(3))
    fn(ctypes.c_int64(n), ip(a), ip(x), ip(y), ip(z))
    return np.stack([x, y, z], -1)


def vox2seq_encode(coords, mode="z_order"):
    """coords (N,3) int -> codes (N,) int32.  mode: 'z_order' | 'hilbert'."""
    coords = np.asarray(coords)
    fn = lib().gvfo_z_order_encode if mode == "z_order" else lib().gvfo_hilbert_encode
    return _vox(fn, coords[:, 0], coords[:, 1], coords[:, 2], 1)


def vox2seq_decode(codes, mode="z_order"):
    fn = lib().gvfo_z_order_decode if mode == "z_order" else lib().gvfo_hilbert_decode
    return _vox(fn, codes, None, None, 3)


# ---- double-precision forward + backward of the rasteriser operator (rast_bwd_oracle.c) -----------------------
def _f64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def _p64(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _scene64(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, H, W, tanfovx, tanfovy,
             kernel_size, scale_modifier, mode, viewmatrix, projmatrix, campos, sh_degree, bg):
    m3 = _f64(means3D); P = m3.shape[0]
    sh = _f64(shs); M = 0 if sh is None else sh.shape[1]
    keep = (m3, sh, _f64(colors_precomp), _f64(np.reshape(opacities, (-1,))), _f64(scales), _f64(rotations),
            _f64(cov3D_precomp), _f64(np.reshape(viewmatrix, (-1,))), _f64(np.reshape(projmatrix, (-1,))), _f64(campos), _f64(bg))
    d = ctypes.c_double
    args = [P, M, int(sh_degree)] + [_p64(a) for a in keep[:7]] + [int(H), int(W), d(tanfovx), d(tanfovy), d(kernel_size),
                                                                   d(scale_modifier), int(mode)] + [_p64(a) for a in keep[7:]]
    return P, M, keep, args


def rast64_forward(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, *, H, W, tanfovx, tanfovy,
                   kernel_size, scale_modifier, mode, viewmatrix, projmatrix, campos, sh_degree, bg):
    """Double-precision forward: dict(color[3,H,W], alpha[H,W], depth[H,W])."""
    P, M, keep, args = _scene64(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, H, W, tanfovx,
                                tanfovy, kernel_size, scale_modifier, mode, viewmatrix, projmatrix, campos, sh_degree, bg)
    color, alpha, depth = np.zeros((3, H, W)), np.zeros((H, W)), np.zeros((H, W))
    rc = lib().gvfo64_forward(*args, _p64(color), _p64(alpha), _p64(depth))
    assert rc == 0
    return dict(color=color, alpha=alpha, depth=depth)


def rast64_backward(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, dL_dcolor, dL_dalpha=None,
                    dL_ddepth=None, *, H, W, tanfovx, tanfovy, kernel_size, scale_modifier, mode, viewmatrix, projmatrix,
                    campos, sh_degree, bg):
    """Double-precision gradients of sum(dL_dcolor*color) + sum(dL_dalpha*alpha) + sum(dL_ddepth*depth):
    dict(means3D, means2D [NDC units], shs | colors_precomp, opacities, scales, rotations | cov3D_precomp)."""
    P, M, keep, args = _scene64(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, H, W, tanfovx,
                                tanfovy, kernel_size, scale_modifier, mode, viewmatrix, projmatrix, campos, sh_degree, bg)
    gc, ga, gd = _f64(dL_dcolor), _f64(dL_dalpha), _f64(dL_ddepth)
    out = dict(means3D=np.zeros((P, 3)), means2D=np.zeros((P, 2)), opacities=np.zeros((P,)))
    g_shs = np.zeros((P, M, 3)) if shs is not None else None
    g_col = np.zeros((P, 3)) if colors_precomp is not None else None
    g_sc = np.zeros((P, 3)) if cov3D_precomp is None else None
    g_ro = np.zeros((P, 4)) if cov3D_precomp is None else None
    g_c6 = np.zeros((P, 6))
    rc = lib().gvfo64_backward(*args, _p64(gc), _p64(ga), _p64(gd), _p64(out["means3D"]), _p64(out["means2D"]), _p64(g_shs),
                               _p64(g_col), _p64(out["opacities"]), _p64(g_sc), _p64(g_ro), _p64(g_c6))
    assert rc == 0
    out.update(shs=g_shs, colors_precomp=g_col, scales=g_sc, rotations=g_ro, cov3D_precomp=g_c6)
    return out


# ---- the backward in its two stages, in fp64 (the reference) and in fp32 (the yardstick: the same file compiled with real = float) ---
class _Prec:
    def __init__(self, dtype, ctype, getlib, prefix):
        self.dtype, self.ctype, self.getlib, self.prefix = dtype, ctype, getlib, prefix

    def fn(self, name):
        return getattr(self.getlib(), self.prefix + name)

    def arr(self, a):
        return None if a is None else np.ascontiguousarray(a, dtype=self.dtype)

    def ptr(self, a):
        return None if a is None else a.ctypes.data_as(ctypes.POINTER(self.ctype))

    def scene(self, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, H, W, tanfovx, tanfovy, kernel_size,
              scale_modifier, mode, viewmatrix, projmatrix, campos, sh_degree, bg):
        m3 = self.arr(means3D); P = m3.shape[0]
        sh = self.arr(shs); M = 0 if sh is None else sh.shape[1]
        keep = (m3, sh, self.arr(colors_precomp), self.arr(np.reshape(opacities, (-1,))), self.arr(scales), self.arr(rotations),
                self.arr(cov3D_precomp), self.arr(np.reshape(viewmatrix, (-1,))), self.arr(np.reshape(projmatrix, (-1,))),
                self.arr(campos), self.arr(bg))
        r = self.ctype
        args = [P, M, int(sh_degree)] + [self.ptr(a) for a in keep[:7]] + \
               [int(H), int(W), r(tanfovx), r(tanfovy), r(kernel_size), r(scale_modifier), int(mode)] + [self.ptr(a) for a in keep[7:]]
        return P, M, keep, args


_P64 = _Prec(np.float64, ctypes.c_double, lib, "gvfo64_")
_P32 = _Prec(np.float32, ctypes.c_float, lib32, "gvfo32_")
_U8 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
_I32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
FLAG_NEAR, FLAG_CLAMPED, FLAG_VISIBLE = 1, 2, 4      # the per-Gaussian flag byte of chain() / project()


def _accumulators(pr, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, dL_dcolor, dL_dalpha, dL_ddepth,
                  subpixel_offset, scene_kw):
    P, M, keep, args = pr.scene(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, **scene_kw)
    so, gc, ga, gd = pr.arr(subpixel_offset), pr.arr(dL_dcolor), pr.arr(dL_dalpha), pr.arr(dL_ddepth)
    acc, acc_abs = np.zeros((P, 10), pr.dtype), np.zeros((P, 10), pr.dtype)
    radii, rects = np.zeros((P,), np.int32), np.zeros((P, 4), np.int32)
    rc = pr.fn("accumulators")(*args, pr.ptr(so), pr.ptr(gc), pr.ptr(ga), pr.ptr(gd), pr.ptr(acc), pr.ptr(acc_abs), _I32(radii), _I32(rects))
    assert rc == 0
    return dict(acc=acc, acc_abs=acc_abs, radii=radii, rects=rects)


def _chain(pr, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, acc, scene_kw):
    P, M, keep, args = pr.scene(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, **scene_kw)
    acc = pr.arr(acc)
    assert acc.shape == (P, 10)
    z = lambda *s: np.zeros(s, pr.dtype)
    out = dict(means3D=z(P, 3), means2D=z(P, 2), opacities=z(P), cov3D_precomp=z(P, 6),
               shs=z(P, M, 3) if shs is not None else None, colors_precomp=z(P, 3) if colors_precomp is not None else None,
               scales=z(P, 3) if cov3D_precomp is None else None, rotations=z(P, 4) if cov3D_precomp is None else None)
    flags = np.zeros((P,), np.uint8)
    rc = pr.fn("chain")(*args, pr.ptr(acc), *[pr.ptr(out[k]) for k in ("means3D", "means2D", "shs", "colors_precomp", "opacities", "scales",
                                                                     "rotations", "cov3D_precomp")], _U8(flags))
    assert rc == 0
    out["flags"] = flags
    return out


def _project(pr, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, txty_fixed, scene_kw):
    P, M, keep, args = pr.scene(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, **scene_kw)
    fixed = pr.arr(txty_fixed)
    out, txty, flags = np.zeros((P, 10), pr.dtype), np.zeros((P, 2), pr.dtype), np.zeros((P,), np.uint8)
    rc = pr.fn("project")(*args, pr.ptr(fixed), pr.ptr(out), _U8(flags), pr.ptr(txty))
    assert rc == 0
    return dict(out=out, flags=flags, txty=txty)


def rast64_accumulators(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, dL_dcolor, dL_dalpha=None,
                        dL_ddepth=None, *, subpixel_offset=None, **scene_kw):
    """Stage 1 of rast64_backward, the blend's backward: dict(acc[P,10], acc_abs[P,10], radii[P], rects[P,4]).  acc = d/d(x, y) [pixels],
    d/d(conic a, b, c), d/d(opacity_eff), d/d(r, g, b), d/d(depth); acc_abs = the same sums over absolute per-(pixel, splat) terms.
    scene_kw: the keyword arguments of rast64_backward.  subpixel_offset: (H, W, 2)."""
    return _accumulators(_P64, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, dL_dcolor, dL_dalpha, dL_ddepth,
                         subpixel_offset, scene_kw)


def rast64_chain(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, acc, **scene_kw):
    """Stage 2 of rast64_backward, the per-Gaussian chain rule from given accumulators (linear in them): the dict of rast64_backward plus
    flags[P] (uint8: FLAG_NEAR | FLAG_CLAMPED | FLAG_VISIBLE)."""
    return _chain(_P64, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, acc, scene_kw)


def rast64_project(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, *, txty_fixed=None, **scene_kw):
    """The per-Gaussian forward the chain rule differentiates: dict(out[P,10] = x, y, conic a, b, c, opacity_eff, r, g, b, depth,
    flags[P], txty[P,2]).  txty_fixed: clamped view coordinates are held at these values (the chain rule gives them no gradient)."""
    return _project(_P64, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, txty_fixed, scene_kw)


def rast32_accumulators(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, dL_dcolor, dL_dalpha=None,
                        dL_ddepth=None, *, subpixel_offset=None, **scene_kw):
    """rast64_accumulators with every operation rounded to fp32: the yardstick."""
    return _accumulators(_P32, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, dL_dcolor, dL_dalpha, dL_ddepth,
                         subpixel_offset, scene_kw)


def rast32_chain(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, acc, *, mutant=0, **scene_kw):
    """rast64_chain with every operation rounded to fp32: the yardstick.  mutant (test-only, 1..7): one line of the chain rule broken."""
    lib32().gvfo32_set_mutant(int(mutant))
    try:
        return _chain(_P32, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, acc, scene_kw)
    finally:
        lib32().gvfo32_set_mutant(0)


def rast32_project(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, *, txty_fixed=None, **scene_kw):
    """rast64_project with every operation rounded to fp32: the yardstick of the forward's projection stage."""
    return _project(_P32, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, txty_fixed, scene_kw)


# ---- the forward's blend on its own (gvfo64_blend / gvfo32_blend): given records over given per-tile lists ----------------------------
PFLAG_ALPHA, PFLAG_T, PFLAG_POWER, PFLAG_CLAMP = 1, 2, 4, 8      # the per-pixel flag byte of blend()


def _blend(pr, rec, ranges, ids, rects, subpixel_offset, bg, H, W, form, want_power):
    rec = pr.arr(rec)
    P = rec.shape[0]
    assert rec.shape == (P, 10)
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)
    if ranges is not None:
        ranges, ids = np.ascontiguousarray(ranges, np.int32), np.ascontiguousarray(ids, np.int32)
        assert ranges.shape == (ntiles, 2) and (ranges[:, 0] <= ranges[:, 1]).all()
        assert ranges.min(initial=0) >= 0 and ranges.max(initial=0) <= ids.shape[0]
        assert ids.size == 0 or (0 <= ids.min() and ids.max() < P)
    else:
        rects = np.ascontiguousarray(rects, np.int32)
        assert rects.shape == (P, 4) and not want_power
    so, bg = pr.arr(subpixel_offset), pr.arr(bg)
    z = lambda *s: np.zeros(s, pr.dtype)
    out = dict(color=z(3, H, W), alpha=z(H, W), depth=z(H, W), s_color=z(3, H, W), s_alpha=z(H, W), s_depth=z(H, W),
               flags=np.zeros((H, W), np.uint8), power=z(ids.shape[0], 16, 16) if want_power else None)
    rc = pr.fn("blend")(P, pr.ptr(rec), None if ranges is None else _I32(ranges), None if ranges is None else _I32(ids),
                        None if ranges is not None else _I32(rects), pr.ptr(so), pr.ptr(bg), int(H), int(W), int(form),
                        *[pr.ptr(out[k]) for k in ("color", "alpha", "depth", "s_color", "s_alpha", "s_depth")], _U8(out["flags"]),
                        pr.ptr(out["power"]))
    assert rc == 0
    return out


def rast64_blend(rec, *, ranges=None, ids=None, rects=None, subpixel_offset=None, bg, H, W, want_power=False):
    """The blend alone, in double precision: records rec[P,10] (x, y, conic a, b, c, opacity_eff, r, g, b, depth: rast64_project's order)
    composited over the per-tile lists ids[ranges[t, 0]:ranges[t, 1]] in the order given, or -- lists = None -- over the lists the function
    builds from the tile rects[P,4] (x0, y0, x1, y1; sorted by fp32 depth bits, then id).  dict(color[3,H,W], alpha, depth, the scales
    s_color[3,H,W] = sum rgb alpha T + T_final bg, s_alpha = sum alpha T, s_depth = sum depth alpha T, flags[H,W] (PFLAG_*), power[D,16,16]
    (want_power, explicit lists: log2 G of every list entry at every pixel of its tile))."""
    return _blend(_P64, rec, ranges, ids, rects, subpixel_offset, bg, H, W, 0, want_power)


def rast32_blend(rec, *, form, ranges=None, ids=None, rects=None, subpixel_offset=None, bg, H, W, want_power=False, mutant=0):
    """rast64_blend in fp32, the yardstick.  form 0: upstream's expression (power from the conic, op * expf(power)); form 1: the device's
    documented algorithm (scaled conic, Cholesky factor in tile-relative coordinates, exp2(log2(op) - s1^2 - s2^2)) in plain C with libm.
    mutant (test-only, 8..11): one blend decision broken."""
    lib32().gvfo32_set_mutant(int(mutant))
    try:
        return _blend(_P32, rec, ranges, ids, rects, subpixel_offset, bg, H, W, form, want_power)
    finally:
        lib32().gvfo32_set_mutant(0)
