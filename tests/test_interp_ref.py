"""The float64 reference of the KNN interpolation loss (tests/interp_ref.py) against the reference's own recorded results, the derived
error bounds against the fp32 torch composition and against a deliberately wrong result, and the stable order among exact ties.
CPU only."""
import numpy as np
import pytest
import torch

import interp_ref as R

from interp_ref import ENCODE_GOLDEN, GOLDEN_CASES, golden_case, padded_queries


def rel(x, y):
    return float(np.abs(np.asarray(x) - np.asarray(y)).max() / max(float(np.abs(np.asarray(y)).max()), 1e-300))


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_ref64_reproduces_the_recorded_float64_results(name):
    gs, static_pc, moving_pc, output, k, adaptive, beta, rec = golden_case(name)
    q, lens = padded_queries(gs)
    ref = R.interp_ref64(q, static_pc, moving_pc, lens, k, beta, adaptive, pred=output[:, :, :q.shape[1]])
    assert abs(float(ref["loss"]) - float(rec["loss64"])) <= 1e-12 * abs(float(rec["loss64"]))
    assert rel(ref["est"].numpy(), rec["est64"]) <= 1e-12
    assert rel(ref["grad"].numpy(), rec["grad64"]) <= 1e-12
    # the reference's own fp32 run sits within the derived bound of it (wherever fp32 cannot have decided differently)
    ok, valid = R.unflagged(ref, lens)
    assert int((valid & ~ok).sum()) <= 0.005 * int(valid.sum())
    err = (torch.from_numpy(rec["est32"]).double() - ref["est"]).abs()
    bound = R.estimate_bound(ref, k, adaptive)
    okb = ok[:, None, :, None].expand_as(err)
    worst = float((err / bound)[okb].max())
    print(f"{name}: worst |est32 - est64| / bound = {worst:.3f}")
    assert worst <= 1.0
    pad = ~valid[:, None, :].expand(err.shape[:3])
    assert float(torch.from_numpy(rec["est32"])[pad].abs().sum()) == 0.0 and float(ref["est"][pad].abs().sum()) == 0.0
    # the elements whose gradient sign fp32 cannot be held to: an exact, recorded count; everywhere else the reference's own fp32
    # gradient has the float64 sign
    sure = R.golden_sure(name, ref, valid, output[:, :, :q.shape[1]], torch.from_numpy(rec["est64"]), k, adaptive)
    assert torch.equal(torch.sign(torch.from_numpy(rec["grad32"])[sure]).double(), torch.sign(torch.from_numpy(rec["grad64"])[sure]))


def test_ref64_reproduces_the_encode_goldens_estimate():
    """`est` of vae_encode_golden.npz came from the reference's compute_delta_interp on the sampled Gaussians (fp32)."""
    z = np.load(ENCODE_GOLDEN)
    q = torch.from_numpy(z["sampled"][..., :3].copy())
    static_pc, delta_pc = torch.from_numpy(z["static_pc"]), torch.from_numpy(z["delta_pc"])
    k, beta = int(z["knn_k"]), float(z["beta"])
    ref = R.interp_ref64(q, static_pc, delta_pc + static_pc[:, None], None, k, beta, True)
    ok, valid = R.unflagged(ref, [q.shape[1]] * q.shape[0])
    assert int((valid & ~ok).sum()) <= 0.005 * int(valid.sum())
    err = (torch.from_numpy(z["est"]).double() - ref["est"]).abs()
    worst = float((err / R.estimate_bound(ref, k, True))[ok[:, None, :, None].expand_as(err)].max())
    print(f"encode golden: worst |est32 - est64| / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("adaptive", [True, False])
@pytest.mark.parametrize("name", ["one", "ragged2", "ragged3", "k16", "k1"])
def test_torch32_composition_is_within_the_derived_bounds(name, adaptive):
    """The bound is not so tight that a correct fp32 evaluation fails it (the large case runs on the device, test_interp_loss_gpu)."""
    c = R.CASES[name]
    q, a, m, _ = R.case_inputs(name)
    ref = R.interp_ref64(q, a, m, c["lens"], c["k"], 7.0, adaptive)
    ok, valid = R.unflagged(ref, c["lens"])
    flagged = int((valid & ~ok).sum())
    assert flagged <= 0.005 * int(valid.sum())
    if name in R.SMALL_CASES:
        assert flagged == 0
    t32 = R.interp_torch32(q, a, m, c["lens"], c["k"], 7.0, adaptive)
    err = (t32["est"].double() - ref["est"]).abs()
    worst = float((err / R.estimate_bound(ref, c["k"], adaptive))[ok[:, None, :, None].expand_as(err)].max())
    print(f"{name} adaptive={adaptive}: flagged {flagged}, worst |est32 - est64| / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("adaptive", [True, False])
def test_bounds_reject_a_weight_off_by_1e_4(adaptive):
    """... and not so loose that a wrong weight passes: one weight of the float64 result changed by 1e-4 relative fails both the
    weight bound and, through the estimate it produces, the estimate bound."""
    c = R.CASES["ragged2"]
    q, a, m, _ = R.case_inputs("ragged2")
    ref = R.interp_ref64(q, a, m, c["lens"], c["k"], 7.0, adaptive)
    b, p = 1, 40
    kbig = int(ref["w"][b, p].argmax())
    w = ref["w"].clone()
    w[b, p, kbig] *= 1.0 + 1e-4
    assert float(((w - ref["w"]).abs() / R.weight_bound(ref, c["k"], adaptive)).max()) > 1.0
    assert float(((ref["w"] - ref["w"]).abs() / R.weight_bound(ref, c["k"], adaptive)).max()) == 0.0
    ik = ref["idx"][b, p]
    mov = m[b].double()[:, ik] - a[b].double()[ik][None]                      # (T, K, 3)
    est = ref["est"].clone()
    est[b, :, p] = (mov * w[b, p][None, :, None]).sum(dim=1)
    ratio = (est - ref["est"]).abs() / R.estimate_bound(ref, c["k"], adaptive)
    assert float(ratio.max()) > 1.0
    assert int((ratio > 1.0).sum()) >= 1 and float(ratio[b, :, :p].sum()) == 0.0


def test_exact_ties_come_out_in_the_stable_order():
    """Lattice inputs: every distance is exact, duplicated anchors tie pairwise, K = 5 splits a pair at the K-th place."""
    q, a, m = R.lattice_case()
    k = 5
    ref = R.interp_ref64(q, a, m, None, k, 7.0, True)
    qd, ad = q.double().numpy()[0], a.double().numpy()[0]
    d = ((qd[:, None, :] - ad[None, :, :]) ** 2).sum(-1)
    d32 = ((q[0][:, None, :] - a[0][None, :, :]) ** 2).sum(-1)
    assert np.array_equal(d32.double().numpy(), d)                            # exact in fp32
    want = np.stack([np.lexsort((np.arange(d.shape[1]), row))[:k] for row in d])
    assert np.array_equal(ref["idx"][0].numpy(), want)
    assert np.array_equal(ref["dist"][0].numpy(), np.take_along_axis(d, want, axis=1))
    half = a.shape[1] // 2
    straddle = int((ref["gap"][0] == 0).sum())
    assert straddle >= q.shape[1] // 2, straddle                               # ties across the K-th place are the rule here
    dk, ik = ref["dist"][0].numpy(), ref["idx"][0].numpy()
    eq = dk[:, 1:] == dk[:, :-1]
    assert eq.any() and (ik[:, 1:][eq] > ik[:, :-1][eq]).all()
    assert (ik[:, 0] < half).all()                                             # of a duplicated pair the first copy comes first
