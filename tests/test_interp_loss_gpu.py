"""KNN interpolation loss on the device (csrc/interp.hip) against the float64 reference of tests/interp_ref.py: neighbour decisions,
element-wise bounds of weights, distances and estimate, the loss value against the fp32 torch composition's own error, the gradient,
exact ties, guard regions, bit-identical relaunch, the recorded results of the reference, the encoder's fused path, and peak memory.
Inputs come from seeded CPU generators; the float64 reference runs on the device in query chunks."""
import ctypes

import numpy as np
import pytest
import torch

import interp_ref as R
from interp_ref import ENCODE_GOLDEN, GOLDEN_CASES, golden_case, padded_queries

pytestmark = pytest.mark.gpu

BETA = 7.0
DEV = "cuda"
_cache = {}


def KI():
    from gvfdiffusion_amd.ops import knn_interp
    return knn_interp


def prepared(name, adaptive):
    """Inputs of a case on the device, its float64 reference, pred = est64 + noise inside a 14-channel tensor, and the fp32 torch
    composition on the same pred (cached per case: the three pred layouts share them)."""
    key = (name, adaptive)
    if key not in _cache:
        _cache.clear()                                        # one case resident at a time
        c = R.CASES[name]
        q, a, m, noise = (t.to(DEV) for t in R.case_inputs(name, C=14))
        ref = R.interp_ref64(q, a, m, c["lens"], c["k"], BETA, adaptive)
        full = noise.clone()
        full[..., :3] += ref["est"].float()
        ref = R.interp_ref64(q, a, m, c["lens"], c["k"], BETA, adaptive, pred=full)
        t32 = R.interp_torch32(q, a, m, c["lens"], c["k"], BETA, adaptive, pred=full[..., :3].contiguous())
        _cache[key] = (c, q, a, m, full, ref, t32)
    return _cache[key]


def flags(ref, lens, name):
    ok, valid = R.unflagged(ref, lens)
    flagged = int((valid & ~ok).sum())
    assert flagged <= 0.005 * int(valid.sum()), f"{flagged} of {int(valid.sum())} queries under the decision threshold"
    if name in R.SMALL_CASES:
        assert flagged == 0
    return ok, valid, flagged


def worst_ratio(err, bound, mask):
    r = (err / bound)[mask]
    return float(r.max()) if r.numel() else 0.0


@pytest.mark.parametrize("adaptive", [True, False])
@pytest.mark.parametrize("name", list(R.CASES))
def test_decisions_weights_distances_estimate(name, adaptive):
    c, q, a, m, _, ref, t32 = prepared(name, adaptive)
    lens, k = c["lens"], c["k"]
    ok, valid, flagged = flags(ref, lens, name)
    idx, w, dist = KI().knn_interp_weights(q, a, lengths=lens, k=k, beta=BETA, adaptive_radius=adaptive, return_dists=True)
    est = KI().delta_interp(q, a, m, lengths=lens, k=k, beta=BETA, adaptive_radius=adaptive)
    assert idx.dtype == torch.int32 and idx.shape == w.shape == dist.shape == ref["w"].shape and est.shape == ref["est"].shape
    # decisions: the neighbours, in order, and which weights the radius cuts
    assert torch.equal(idx[ok].long(), ref["idx"][ok])
    assert torch.equal(w[ok] == 0, ref["w"][ok] == 0)
    # element-wise bounds, nothing exempt among the unflagged queries
    okk = ok[..., None].expand_as(w)
    oke = ok[:, None, :, None].expand_as(est)
    rw = worst_ratio((w.double() - ref["w"]).abs(), R.weight_bound(ref, k, adaptive), okk)
    rd = worst_ratio((dist.double() - ref["dist"]).abs(), R.dist_bound(ref), okk)
    re = worst_ratio((est.double() - ref["est"]).abs(), R.estimate_bound(ref, k, adaptive), oke)
    rt = worst_ratio((t32["est"].double() - ref["est"]).abs(), R.estimate_bound(ref, k, adaptive), oke)
    print(f"{name} adaptive={adaptive}: flagged {flagged}; worst |err| / bound: w {rw:.3f}, dist {rd:.3f}, est {re:.3f} (torch fp32 est {rt:.3f})")
    assert rw <= 1.0 and rd <= 1.0 and re <= 1.0
    assert rt <= 1.0                                          # the yardstick passes its own bound on this input
    # padded queries: exactly zero
    pad = ~valid
    assert float(w[pad].abs().sum()) == 0.0 and float(est[pad[:, None, :].expand(est.shape[:3])].abs().sum()) == 0.0
    # the queries left out above are still sane
    out = valid & ~ok
    if out.any():
        wo, eo = w[out], est.permute(0, 2, 1, 3)[out]                     # (n, K), (n, T, 3)
        assert torch.isfinite(wo).all() and torch.isfinite(eo).all() and (idx[out] >= 0).all() and (idx[out] < c["N"]).all()
        # fp32 rounding of the K normalised weights and of the K-term sum: a few u each, 32 u covers K <= 16
        slack = 1 + 32 * R.U
        assert (wo >= 0).all() and (wo <= 1).all() and (wo.sum(dim=1) <= slack).all()
        # a convex combination of the motions of the neighbours the device took: within max_k |m_k - a_k| of zero
        b_of = torch.nonzero(out)[:, 0]
        ii = idx[out].long()                                                 # (n, K)
        mov = m[b_of[:, None], :, ii] - a[b_of[:, None], ii][:, :, None]     # (n, K, T, 3)
        lim = mov.abs().amax(dim=(1, 3))                                      # (n, T)
        assert (eo.abs() <= lim[..., None] * slack).all()


@pytest.mark.parametrize("layout", ["view14", "dense3", "full14"])
@pytest.mark.parametrize("adaptive", [True, False])
@pytest.mark.parametrize("name", list(R.CASES))
def test_loss_and_gradient(name, adaptive, layout):
    """Loss value and gradient (rule 5), pred as a [..., :3] view of a 14-channel tensor, dense, and as the 14-channel tensor itself."""
    c, q, a, m, full, ref, t32 = prepared(name, adaptive)
    lens, k, T = c["lens"], c["k"], c["T"]
    ok, valid, _ = flags(ref, lens, name)
    leaf = (full[..., :3].contiguous() if layout == "dense3" else full.clone()).requires_grad_(True)
    pred = leaf[..., :3] if layout == "view14" else leaf
    loss, est = KI().interpolation_l1(pred, q, a, m, lengths=lens, k=k, beta=BETA, adaptive_radius=adaptive, return_est=True)
    assert loss.dim() == 0 and not est.requires_grad
    assert torch.equal(est, KI().delta_interp(q, a, m, lengths=lens, k=k, beta=BETA, adaptive_radius=adaptive))
    l64, l32, lh = float(ref["loss"]), float(t32["loss"]), float(loss)
    tol = max(2 * abs(l32 - l64), 1e-7 * abs(l64))
    print(f"{name} adaptive={adaptive} {layout}: loss64 {l64:.10g} hip {lh:.10g} torch32 {l32:.10g} |hip-64| {abs(lh - l64):.3g} tol {tol:.3g}")
    assert abs(lh - l64) <= tol
    (3 * loss).backward()
    g3 = leaf.grad
    leaf.grad = None
    loss2 = KI().interpolation_l1(pred, q, a, m, lengths=lens, k=k, beta=BETA, adaptive_radius=adaptive)
    assert torch.equal(loss2, loss)                                         # same bits on a second launch
    loss2.backward()
    g = leaf.grad
    assert g.shape == leaf.shape
    if g.shape[-1] > 3:
        assert float(g[..., 3:].abs().sum()) == 0.0 and float(g3[..., 3:].abs().sum()) == 0.0
    g, g3 = g[..., :3], g3[..., :3]
    cnt = 3.0 * T * sum(lens)
    mag = np.float32(1.0 / cnt)
    tmag = float(t32["grad"].abs().max())
    assert abs(np.float32(tmag) - mag) <= np.spacing(mag)                   # at most 1 ulp from torch's value
    nz = g != 0
    assert ((g[nz].abs() - float(mag)).abs() <= float(np.spacing(mag))).all()
    assert ((g[nz].abs() - tmag).abs() <= float(np.spacing(mag))).all()
    # an incoming gradient scales the result linearly
    assert torch.equal(g3 != 0, nz) and ((g3 - 3 * g).abs() <= 3 * float(np.spacing(mag)) * 2).all()
    # padded queries: exactly zero
    pad = (~valid)[:, None, :].expand(g.shape[:3])
    assert float(g[pad].abs().sum()) == 0.0
    # the sign is the reference's wherever pred is further from the float64 estimate than fp32 can move the estimate
    diff = (full[..., :3].double() - ref["est"]).abs()
    sure = (diff > R.estimate_bound(ref, k, adaptive)) & ok[:, None, :, None]
    oke = ok[:, None, :, None].expand_as(diff)
    unsure = int((oke & ~sure).sum())
    assert unsure <= 0.001 * int(oke.sum()), unsure
    assert torch.equal(torch.sign(g[sure]).double(), torch.sign(ref["grad"][sure]))
    assert (g[sure] != 0).all()


def test_zero_motion_gives_exact_zeros():
    c = R.CASES["ragged2"]
    q, a, m, _ = (t.to(DEV) for t in R.case_inputs("ragged2"))
    m = a[:, None].expand_as(m).contiguous()
    pred = torch.zeros((2, c["T"], max(c["lens"]), 14), device=DEV, requires_grad=True)
    loss, est = KI().interpolation_l1(pred, q, a, m, lengths=c["lens"], k=c["k"], return_est=True)
    loss.backward()
    assert float(loss) == 0.0 and float(est.abs().sum()) == 0.0 and float(pred.grad.abs().sum()) == 0.0


def test_exact_ties_take_the_lower_index_first():
    """The lattice case of test_interp_ref on the device: distances are exact in fp32, so the indices must equal the stable order for
    EVERY query, tied at the K-th place or not; the margin flag still guards the weights."""
    q, a, m = (t.to(DEV) for t in R.lattice_case())
    k = 5
    for adaptive in (True, False):
        ref = R.interp_ref64(q, a, m, None, k, BETA, adaptive)
        assert int((ref["gap"] == 0).sum()) >= q.shape[1] // 2
        idx, w, dist = KI().knn_interp_weights(q, a, k=k, beta=BETA, adaptive_radius=adaptive, return_dists=True)
        assert torch.equal(idx.long(), ref["idx"])
        assert torch.equal(dist.double(), ref["dist"])                      # exact
        okw = (ref["margin"] > R.FLAG)[..., None].expand_as(w)
        assert int(okw[..., 0].sum()) >= 0.9 * q.shape[1]
        assert worst_ratio((w.double() - ref["w"]).abs(), R.weight_bound(ref, k, adaptive), okw) <= 1.0
        est = KI().delta_interp(q, a, m, k=k, beta=BETA, adaptive_radius=adaptive)
        oke = (ref["margin"] > R.FLAG)[:, None, :, None].expand_as(est)
        assert worst_ratio((est.double() - ref["est"]).abs(), R.estimate_bound(ref, k, adaptive), oke) <= 1.0


def _guarded(n, dtype, sentinel, guard=1024):
    buf = torch.full((guard + n + guard,), sentinel, dtype=dtype, device=DEV)
    return buf, ctypes.c_void_p(buf.data_ptr() + guard * buf.element_size()), guard


def _intact(buf, guard, sentinel):
    return bool((buf[:guard] == sentinel).all()) and bool((buf[-guard:] == sentinel).all())


def test_guard_regions_and_relaunch_bits():
    """Every output of every entry point, written through the C ABI between sentinel regions: nothing outside the output changes,
    the channels >= 3 of a strided gradient stay untouched, and a second launch gives the same bits."""
    from gvfdiffusion_amd import _lib
    KI()
    L = _lib.lib()
    c = R.CASES["ragged3"]
    lens, N, T, k = c["lens"], c["N"], c["T"], c["k"]
    q, a, m, noise = (t.to(DEV).contiguous() for t in R.case_inputs("ragged3", C=14))
    B, P = q.shape[0], q.shape[1]
    ln = torch.tensor(lens, dtype=torch.int32, device=DEV)
    s = _lib.current_stream(torch.device(DEV))
    runs = []
    for _ in range(2):
        idx, pidx, G = _guarded(B * P * k, torch.int32, -77)
        w, pw, _ = _guarded(B * P * k, torch.float32, -7.5)
        dist, pdist, _ = _guarded(B * P * k, torch.float32, -7.5)
        est, pest, _ = _guarded(B * T * P * 3, torch.float32, -7.5)
        est2, pest2, _ = _guarded(B * T * P * 3, torch.float32, -7.5)
        sign, psign, _ = _guarded(B * T * P, torch.uint8, 0xEE)
        grad, pgrad, _ = _guarded(B * T * P * 14, torch.float32, -7.5)
        loss, ploss, _ = _guarded(1, torch.float32, -7.5)
        _lib.check(L.gvf_knn_interp_weights(_lib.ptr(q), _lib.ptr(ln), _lib.ptr(a), B, P, N, k, BETA, 1, pidx, pw, pdist, s), "weights")
        _lib.check(L.gvf_knn_interp_apply(pidx, pw, _lib.ptr(a), _lib.ptr(m), B, T, P, N, k, pest, s), "apply")
        nb = ctypes.c_size_t(0)
        _lib.check(L.gvf_interp_loss_scratch_bytes(B, T, P, ctypes.byref(nb)), "scratch")
        scratch, pscratch, _ = _guarded(nb.value, torch.uint8, 0xEE)
        _lib.check(L.gvf_interp_loss_forward(_lib.ptr(noise), 14, pidx, pw, _lib.ptr(a), _lib.ptr(m), _lib.ptr(ln), B, T, P, N, k, ploss, pest2,
                                             psign, pscratch, nb.value, s), "forward")
        one = torch.ones(1, device=DEV)
        _lib.check(L.gvf_interp_loss_backward(psign, _lib.ptr(one), _lib.ptr(ln), B, T, P, pgrad, 14, 3, s), "backward")
        torch.cuda.synchronize()
        for buf, sent in ((idx, -77), (w, -7.5), (dist, -7.5), (est, -7.5), (est2, -7.5), (sign, 0xEE), (grad, -7.5), (loss, -7.5),
                          (scratch, 0xEE)):
            assert _intact(buf, G, sent)
        rows = grad[G:-G].view(B * T * P, 14)
        assert bool((rows[:, 3:] == -7.5).all()) and bool((rows[:, :3] != -7.5).all())
        assert torch.equal(est[G:-G], est2[G:-G]) and bool((sign[G:-G] != 0xEE).all())
        runs.append([t[G:-G].clone() for t in (idx, w, dist, est, sign, grad, loss)])
        # the zero fill of further channels is opt-in per call
        _lib.check(L.gvf_interp_loss_backward(psign, _lib.ptr(one), _lib.ptr(ln), B, T, P, pgrad, 14, 9, s), "backward")
        torch.cuda.synchronize()
        rows = grad[G:-G].view(B * T * P, 14)
        assert bool((rows[:, 3:9] == 0).all()) and bool((rows[:, 9:] == -7.5).all()) and _intact(grad, G, -7.5)
    for x, y in zip(*runs):
        assert torch.equal(x, y)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_recorded_reference_results_through_training(name):
    from gvfdiffusion_amd import training
    gs, static_pc, moving_pc, output, k, adaptive, beta, rec = golden_case(name)
    q, lens = padded_queries(gs)
    ref = R.interp_ref64(q, static_pc, moving_pc, lens, k, beta, adaptive, pred=output)
    ok, valid = R.unflagged(ref, lens)
    assert int((valid & ~ok).sum()) == 0
    out = output.to(DEV).requires_grad_(True)
    res = training.interpolation_loss([g.to(DEV) for g in gs], static_pc.to(DEV), moving_pc.to(DEV), out, knn_k=k, adaptive_radius=adaptive,
                                      beta=beta)
    assert isinstance(res, tuple) and len(res) == 3
    loss, d, est = res
    assert set(d) == {"deformation_xyz_loss"} and tuple(d["deformation_xyz_loss"].shape) == (1,) and not d["deformation_xyz_loss"].requires_grad
    assert float(d["deformation_xyz_loss"]) == float(loss) and tuple(est.shape) == rec["est64"].shape and not est.requires_grad
    l64 = float(rec["loss64"])
    assert abs(float(loss) - l64) <= max(2 * abs(float(rec["loss32"]) - l64), 1e-7 * abs(l64))
    err = (est.cpu().double() - torch.from_numpy(rec["est64"])).abs()
    ratio = worst_ratio(err, R.estimate_bound(ref, k, adaptive), ok[:, None, :, None].expand_as(err))
    print(f"{name}: loss {float(loss):.10g} (float64 {l64:.10g}), worst |est - est64| / bound {ratio:.3f}")
    assert ratio <= 1.0
    assert float(est.cpu()[(~valid)[:, None, :].expand(est.shape[:3])].abs().sum()) == 0.0
    loss.backward()
    g = out.grad.cpu()
    assert g.shape == output.shape and float(g[..., 3:].abs().sum()) == 0.0
    g64 = torch.from_numpy(rec["grad64"])
    # every valid element but the fixture's recorded under-bound ones (an exact count, tests/interp_ref.py) has the float64 sign
    sure = R.golden_sure(name, ref, valid, output, torch.from_numpy(rec["est64"]), k, adaptive)
    assert torch.equal(torch.sign(g[..., :3][sure]).double(), torch.sign(g64[sure]))
    mag = np.float32(float(g64.abs().max()))
    nz = g[..., :3] != 0
    assert ((g[..., :3][nz].abs() - float(mag)).abs() <= float(np.spacing(mag))).all()
    assert float(g[..., :3][(~valid)[:, None, :].expand(g.shape[:3])].abs().sum()) == 0.0


def test_encoder_fused_path_matches_the_torch_path():
    from gvfdiffusion_amd.model.autoencoder import GSKLTemporalVariationalAutoEncoder as VAE
    z = np.load(ENCODE_GOLDEN)
    q = torch.from_numpy(z["sampled"][..., :3].copy()).to(DEV)
    static_pc, delta_pc = torch.from_numpy(z["static_pc"]).to(DEV), torch.from_numpy(z["delta_pc"]).to(DEV)
    moving = delta_pc + static_pc[:, None]
    k, beta = int(z["knn_k"]), float(z["beta"])
    ref = R.interp_ref64(q, static_pc, moving, None, k, beta, True)
    ok, valid = R.unflagged(ref, [q.shape[1]] * q.shape[0])
    assert int((valid & ~ok).sum()) <= 0.005 * int(valid.sum())
    plain = VAE.compute_delta_interp(q, static_pc, moving, knn_k=k, beta=beta)
    fused = VAE.compute_delta_interp(q, static_pc, moving, knn_k=k, beta=beta, fused=True)
    assert fused.shape == plain.shape and fused.dtype == plain.dtype
    bound = R.estimate_bound(ref, k, True)
    oke = ok[:, None, :, None].expand_as(bound)
    rf = worst_ratio((fused.double() - ref["est"]).abs(), bound, oke)
    rp = worst_ratio((plain.double() - ref["est"]).abs(), bound, oke)
    rg = worst_ratio((torch.from_numpy(z["est"]).to(DEV).double() - ref["est"]).abs(), bound, oke)
    print(f"encode golden: worst |err| / bound: fused {rf:.3f}, torch path {rp:.3f}, recorded {rg:.3f}")
    assert rf <= 1.0 and rp <= 1.0 and rg <= 1.0


def test_full_size_estimate_and_loss():
    """(1, 262144, 8192, 24, 8): estimate and loss against the float64 reference evaluated in query chunks."""
    lens, N, T, k = [262144], 8192, 24, 8
    q, a, m, noise = (t.to(DEV) for t in R.make_case(7, lens, N, T, C=14))
    ref = R.interp_ref64(q, a, m, lens, k, BETA, True)
    full = noise
    full[..., :3] += ref["est"].float()
    ok, valid, flagged = flags(ref, lens, "full")
    cnt = 3.0 * T * lens[0]
    l64 = float((full[..., :3].double() - ref["est"]).abs().sum() / cnt)
    t32 = R.interp_torch32(q, a, m, lens, k, BETA, True, chunk=32768)["est"]
    l32 = float((full[..., :3] - t32).abs().sum() / np.float32(cnt))
    loss, est = KI().interpolation_l1(full[..., :3], q, a, m, lengths=lens, k=k, beta=BETA, return_est=True)
    oke = ok[:, None, :, None].expand_as(est)
    bound = R.estimate_bound(ref, k, True)
    re = worst_ratio((est.double() - ref["est"]).abs(), bound, oke)
    rt = worst_ratio((t32.double() - ref["est"]).abs(), bound, oke)
    tol = max(2 * abs(l32 - l64), 1e-7 * abs(l64))
    print(f"full size: flagged {flagged}; worst |est - est64| / bound {re:.3f} (torch fp32 {rt:.3f}); loss64 {l64:.10g} hip {float(loss):.10g} "
          f"torch32 {l32:.10g} tol {tol:.3g}")
    assert re <= 1.0 and rt <= 1.0
    assert abs(float(loss) - l64) <= tol


def test_peak_memory_has_no_distance_matrix():
    """(1, 65536, 8192, 24, 8): one forward + backward may allocate its outputs (loss, gradient), idx, w, the sign bytes and 16 MB;
    the distance matrix alone would be 2.1 GB."""
    B, P, N, T, k = 1, 65536, 8192, 24, 8
    q, a, m, noise = (t.to(DEV) for t in R.make_case(8, [P], N, T, C=14))
    leaf = noise.requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = KI().interpolation_l1(leaf, q, a, m, k=k)
    loss.backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    allowed = 4 + B * T * P * 14 * 4 + B * P * k * 8 + B * T * P + (16 << 20)     # loss, gradient, idx + w, sign bytes
    print(f"peak memory rise {rise / 2**20:.1f} MiB, allowed {allowed / 2**20:.1f} MiB")
    assert rise <= allowed
    assert leaf.grad is not None and float(leaf.grad[..., 3:].abs().sum()) == 0.0
