"""Fused clip + AdamW + EMA step on the MI355X (ops/optim.py::FusedAdamW, csrc/optim.hip) against the fp64 formula.

Inputs (tests/optim_util.py): a ragged tensor set around the chunk length C -- 1 .. 1025, C-1, C, C+1, 2C+7, an empty tensor, one of
3 * 2^20 + 5 elements over many chunks and a contiguous view at a 4-byte offset (the scalar path) -- in two groups (lr 1e-4 / 1e-5, weight
decay 0.01 / 0), two EMAs (0.9999, 0.999), parameters N(0, 0.05^2), gradients N(0, 1) x 10^U(-8, 0), non-zero moments.

The bars are staged and derived from the rounding count, E = 2^-24: m' within 4E(|b1 m| + |(1-b1) gc|), v' within
4E(|b2 v| + |(1-b2) gc^2|), p' within 8E(|p (1 - lr wd)| + |u|) with u in fp64 from the kernel's m', v', each EMA within
4E(|r e| + |(1-r) p'|); grad_norm within 2^-22 relative of the fp64 norm; clip_coef equal to torch's formula on that fp32 norm."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import optim_util as U  # noqa: E402

pytestmark = pytest.mark.gpu


def _setup(cuda, step0=7, max_grad_norm=None, big=True, grad_seed=1, grad_scale=1.0, sigma=None):
    """A FusedAdamW over the ragged set with moments, step count and gradients in place.  Returns (opt, params, grads, group index)."""
    from gvfdiffusion_amd.ops.optim import FusedAdamW, chunk_len
    params = U.make_params(cuda, chunk_len(), big=big)
    opt = FusedAdamW(U.groups_of(params), betas=U.BETAS, eps=U.EPS, ema_rates=U.EMA_RATES, max_grad_norm=max_grad_norm)
    ms, vs = U.make_moments(params)
    U.set_state(opt, params, step0, ms, vs)
    # EMAs that differ from the parameters, so that both terms of their update matter
    g = torch.Generator().manual_seed(5)
    for k in range(len(U.EMA_RATES)):
        for e in opt.ema_params(k):
            e.add_((0.01 * torch.randn(e.numel(), generator=g)).to(cuda).view(e.shape))
    grads = U.make_grads(params, seed=grad_seed, sigma=sigma)
    for p, gr in zip(params, grads):
        p.grad.copy_(gr * grad_scale)
    assert opt.flat_grads.owns(params)
    return opt, params, grads, U.group_index(params)


@pytest.mark.parametrize("step0", [0, 7, 999])
def test_one_step_staged_fp64_conformance(cuda, step0):
    opt, params, grads, groups = _setup(cuda, step0=step0, max_grad_norm=None)
    before = U.snapshot(opt, params)
    opt.step()
    after = U.snapshot(opt, params)
    assert int(after["found_inf"]) == 0 and int(after["step"]) == step0 + 1
    U.assert_within_bars(U.staged_errors(before, after, grads, groups, step0 + 1), f"step0={step0}")
    ref = U.norm_f64(grads)
    got = float(after["grad_norm"])
    print(f"grad_norm {got!r} fp64 {ref!r} relative error {abs(got - ref) / ref:.3e} (bar {2.0 ** -22:.3e})")
    assert abs(got - ref) <= 2.0 ** -22 * ref
    assert float(after["clip_coef"]) == 1.0
    # every element moved, and the element in front of the view at the 4-byte offset is intact
    assert float(params[-1].guard_base[0]) == U.GUARD
    assert all(not torch.equal(a, b) for a, b in zip(before["p"], after["p"]) if a.numel())
    assert all(not torch.equal(a, b) for a, b in zip(before["ema"][0], after["ema"][0]) if a.numel())


def test_clip_below_and_above_the_norm(cuda):
    opt, params, grads, groups = _setup(cuda, max_grad_norm=1.0)
    before = U.snapshot(opt, params)
    opt.step()
    clipped = U.snapshot(opt, params)
    norm32 = clipped["grad_norm"].cpu()
    assert float(norm32) > 10.0, "the clip must bite for this test to mean anything"
    want = U.torch_clip_coef(norm32, 1.0)
    assert clipped["clip_coef"].cpu().view(torch.int32) == want.view(torch.int32), (float(clipped["clip_coef"]), float(want))
    assert float(want) < 0.1
    U.assert_within_bars(U.staged_errors(before, clipped, grads, groups, 8), "clipped")      # gc uses the kernel's clip_coef
    # above the norm: bit-identical to no clipping at all
    runs = []
    for max_norm in (1e6, None):
        opt, params, grads, groups = _setup(cuda, max_grad_norm=max_norm)
        opt.step()
        runs.append(U.snapshot(opt, params))
    assert float(runs[0]["clip_coef"]) == 1.0
    assert U.snapshots_equal(runs[0], runs[1])
    assert not all(torch.equal(a, b) for a, b in zip(runs[0]["p"], clipped["p"]))


def test_loss_scale_is_bit_transparent(cuda):
    opt, params, _, _ = _setup(cuda, max_grad_norm=1.0)
    opt.step()
    plain = U.snapshot(opt, params)
    opt, params, _, _ = _setup(cuda, max_grad_norm=1.0, grad_scale=1024.0)
    opt.step(inv_scale=torch.tensor([1.0 / 1024.0], device=cuda))
    scaled = U.snapshot(opt, params)
    assert U.snapshots_equal(plain, scaled)
    with pytest.raises(ValueError):
        opt.step(inv_scale=torch.tensor([1.0, 2.0], device=cuda))


@pytest.mark.parametrize("poison", ["inf_in_large", "nan_in_single"])
def test_non_finite_gradient_skips_the_step_but_not_the_emas(cuda, poison):
    step0 = 7
    opt, params, grads, groups = _setup(cuda, step0=step0, max_grad_norm=1.0)
    sizes = [p.numel() for p in params]
    if poison == "inf_in_large":
        i = sizes.index(max(sizes))
        params[i].grad.view(-1)[sizes[i] // 2] = float("inf")
    else:
        i = sizes.index(1)
        params[i].grad.view(-1)[0] = float("nan")
    before = U.snapshot(opt, params)
    opt.step()
    after = U.snapshot(opt, params)
    assert int(after["found_inf"]) == 1 and not torch.isfinite(after["grad_norm"])
    assert int(after["step"]) == step0
    for key in ("p", "m", "v"):
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before[key], after[key])), key
    errs = U.staged_errors(before, after, grads, groups, step0, skipped=True)
    print(f"{poison}: EMA error after the skipped step {errs['ema']:.3f} E x magnitude (bar 4)")
    assert errs["ema"] <= U.BARS["ema"]
    assert all(not torch.equal(a, b) for a, b in zip(before["ema"][1], after["ema"][1]) if a.numel())
    # the next finite step is step0 + 1
    opt.zero_grad()
    for p, g in zip(params, grads):
        p.grad.copy_(g)
    opt.step()
    last = U.snapshot(opt, params)
    assert int(last["found_inf"]) == 0 and int(last["step"]) == step0 + 1
    U.assert_within_bars(U.staged_errors(after, last, grads, groups, step0 + 1), f"{poison}, next step")


def test_bitwise_determinism_across_runs_and_streams(cuda):
    runs = []
    for stream in (None, None, torch.cuda.Stream(device=cuda)):
        opt, params, _, _ = _setup(cuda, max_grad_norm=1.0)
        if stream is None:
            opt.step()
        else:
            stream.wait_stream(torch.cuda.current_stream(cuda))
            with torch.cuda.stream(stream):
                opt.step()
            torch.cuda.current_stream(cuda).wait_stream(stream)
        runs.append(U.snapshot(opt, params))
    assert U.snapshots_equal(runs[0], runs[1]), "two runs on the default stream differ"
    assert U.snapshots_equal(runs[0], runs[2]), "the run on a side stream differs"


def _ema_loop(emas, params, rates):
    """The reference's update_ema: targ.mul_(rate).add_(src, alpha=1 - rate) per tensor and rate."""
    for views, r in zip(emas, rates):
        for e, p in zip(views, params):
            e.mul_(r).add_(p.detach(), alpha=1 - r)


def test_twenty_steps_track_fp64_as_well_as_stock_adamw(cuda):
    """Fused, stock torch.optim.AdamW (fp32) and an fp64 trajectory under one LambdaLR warm-up and the same seeded gradients N(0, 1e-2^2):
    the fused maximum element-wise error in p and in the EMA is at most 2x the stock optimizer's (both are fp32 evaluations that differ in
    rounding order only)."""
    from gvfdiffusion_amd.ops.optim import FusedAdamW, chunk_len
    from torch.optim.lr_scheduler import LambdaLR
    params = U.make_params(cuda, chunk_len(), big=True)
    p32 = [torch.nn.Parameter(p.detach().clone()) for p in params]
    p64 = [torch.nn.Parameter(p.detach().double()) for p in params]
    fused = FusedAdamW(U.groups_of(params), betas=U.BETAS, eps=U.EPS, ema_rates=U.EMA_RATES)
    stock = torch.optim.AdamW(U.groups_of(p32), betas=U.BETAS, eps=U.EPS)
    exact = torch.optim.AdamW(U.groups_of(p64), betas=U.BETAS, eps=U.EPS)
    e32 = [[p.detach().clone() for p in p32] for _ in U.EMA_RATES]
    e64 = [[p.detach().clone() for p in p64] for _ in U.EMA_RATES]
    warm = lambda s: min(1.0, (s + 1) / 10.0)  # noqa: E731
    scheds = [LambdaLR(o, warm) for o in (fused, stock, exact)]
    for step in range(20):
        grads = U.make_grads(params, seed=1000 + step, sigma=1e-2)
        fused.zero_grad()
        for p, a, b, g in zip(params, p32, p64, grads):
            p.grad.copy_(g)
            a.grad = g.clone()
            b.grad = g.double()
        fused.step()
        stock.step()
        exact.step()
        _ema_loop(e32, p32, U.EMA_RATES)
        _ema_loop(e64, p64, U.EMA_RATES)
        for s in scheds:
            s.step()
    assert int(fused.step_count) == 20 and fused.param_groups[0]["lr"] == stock.param_groups[0]["lr"]

    def worst(xs, refs):
        return max(float((x.detach().double() - r.detach()).abs().max()) for x, r in zip(xs, refs) if x.numel())

    err_p_fused, err_p_stock = worst(params, p64), worst(p32, p64)
    print(f"20 steps, max |p - p64|: fused {err_p_fused:.3e}, stock AdamW {err_p_stock:.3e}, ratio {err_p_fused / err_p_stock:.3f}")
    assert err_p_stock > 0 and max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(params, p32) if p.numel()) < 1e-5
    for k in range(len(U.EMA_RATES)):
        ef, es = worst(U.ema_views(fused, params, k), e64[k]), worst(e32[k], e64[k])
        print(f"20 steps, EMA {U.EMA_RATES[k]}: max |e - e64| fused {ef:.3e}, stock loop {es:.3e}, ratio {ef / es:.3f}")
        assert ef <= 2.0 * es
    assert err_p_fused <= 2.0 * err_p_stock      # measured on an MI355X: ratio 1.000 for p and for both EMAs (profiles/r13_optim_step.txt)


def test_state_interchange_with_stock_adamw(cuda):
    """Three steps of stock AdamW -> its state_dict loads into FusedAdamW -> one more step of each from the same gradients agrees within
    the staged bars; FusedAdamW's state_dict loads into a stock AdamW."""
    from gvfdiffusion_amd.ops.optim import FusedAdamW, chunk_len
    p32 = U.make_params(cuda, chunk_len(), big=False)
    stock = torch.optim.AdamW(U.groups_of(p32), betas=U.BETAS, eps=U.EPS)
    for step in range(3):
        for p, g in zip(p32, U.make_grads(p32, seed=50 + step)):
            p.grad = g
        stock.step()
    params = [torch.nn.Parameter(p.detach().clone()) for p in p32]
    fused = FusedAdamW(U.groups_of(params), betas=U.BETAS, eps=U.EPS, ema_rates=U.EMA_RATES)
    fused.load_state_dict(stock.state_dict())
    assert int(fused.step_count) == 3
    for p, q in zip(params, p32):
        assert torch.equal(fused.state[p]["exp_avg"], stock.state[q]["exp_avg"]) and torch.equal(fused.state[p]["exp_avg_sq"], stock.state[q]["exp_avg_sq"])
    grads = U.make_grads(p32, seed=60)
    before = U.snapshot(fused, params)
    for p, q, g in zip(params, p32, grads):
        p.grad.copy_(g)
        q.grad = g.clone()
    fused.step()
    stock.step()
    after = U.snapshot(fused, params)
    U.assert_within_bars(U.staged_errors(before, after, grads, U.group_index(params), 4), "fused after load")
    # fused against stock, in the same units: both sit within the bars of the same fp64 values
    as_stock = dict(after, p=[q.detach().clone() for q in p32], m=[stock.state[q]["exp_avg"] for q in p32],
                    v=[stock.state[q]["exp_avg_sq"] for q in p32], ema=[])
    b1, b2 = U.BETAS
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    for i, g in enumerate(grads):
        gc = g.double()
        lr, wd = U.LRS[i % 2], U.WDS[i % 2]
        m0, v0, p0 = before["m"][i].double(), before["v"][i].double(), before["p"][i].double()
        m1, v1 = b1 * m0 + (1 - b1) * gc, b2 * v0 + (1 - b2) * gc * gc
        u = (lr / (1 - b1 ** 4)) * m1 / (v1.sqrt() / (1 - b2 ** 4) ** 0.5 + U.EPS)
        for key, x, y, mag in (("m", after["m"][i], as_stock["m"][i], (b1 * m0).abs() + ((1 - b1) * gc).abs()),
                               ("v", after["v"][i], as_stock["v"][i], (b2 * v0).abs() + ((1 - b2) * gc * gc).abs()),
                               ("p", after["p"][i], as_stock["p"][i], (p0 * (1 - lr * wd)).abs() + u.abs())):
            worst[key] = max(worst[key], U._worst((x.double() - y.double()).abs(), U.E * mag))
    U.assert_within_bars(worst, "fused against stock AdamW")
    # the reverse direction
    sd = fused.state_dict()
    assert "ema" in sd and len(sd["ema"]["params"]) == 2
    other = torch.optim.AdamW(U.groups_of([torch.nn.Parameter(p.detach().clone()) for p in params]), betas=U.BETAS, eps=U.EPS)
    other.load_state_dict(copy.deepcopy(sd))             # a state dict holds references: a copy keeps the two optimizers apart
    q0 = other.param_groups[0]["params"][0]
    assert float(other.state[q0]["step"]) == 4.0 and torch.equal(other.state[q0]["exp_avg"], fused.state[params[0]]["exp_avg"])
    for g in other.param_groups:
        for q in g["params"]:
            q.grad = torch.zeros_like(q)
    other.step()                                             # the loaded groups carry every key a stock step reads
    # and back into a fresh fused optimizer, EMAs included
    again = FusedAdamW(U.groups_of([torch.nn.Parameter(p.detach().clone()) for p in params]), betas=U.BETAS, eps=U.EPS, ema_rates=U.EMA_RATES)
    again.load_state_dict(copy.deepcopy(sd))
    assert int(again.step_count) == 4
    assert all(torch.equal(a, b) for a, b in zip(again.ema_params(1), fused.ema_params(1)))


def test_train_step_with_fused_adamw(cuda):
    from gvfdiffusion_amd.ops.optim import FusedAdamW
    from gvfdiffusion_amd.training import train_step
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(16, 64), torch.nn.GELU(), torch.nn.Linear(64, 4)).to(cuda)
    frozen = copy.deepcopy(net)
    x = torch.randn(256, 16, device=cuda)
    y = torch.randn(256, 4, device=cuda)
    params = list(net.parameters())
    opt = FusedAdamW(params, lr=1e-2, weight_decay=0.0, ema_rates=(0.99,))
    loss_fn = lambda: torch.nn.functional.mse_loss(net(x), y)  # noqa: E731
    infos = [train_step(params, opt, loss_fn, max_grad_norm=0.5) for _ in range(10)]
    assert infos[-1]["loss"] < infos[0]["loss"], [i["loss"] for i in infos]
    assert all(i["found_inf"] == 0 for i in infos) and all(i["collectives"] == 0 for i in infos)
    assert opt.flat_grads.owns(params) and opt.max_grad_norm == 0.5
    # the first step's norm against clip_grad_norm_ on a clone of the initial model
    torch.nn.functional.mse_loss(frozen(x), y).backward()
    ref64 = sum(float(p.grad.double().square().sum()) for p in frozen.parameters()) ** 0.5
    ref32 = float(torch.nn.utils.clip_grad_norm_(list(frozen.parameters()), 0.5))
    got = infos[0]["grad_norm"]
    print(f"train_step grad_norm {got!r}, fp64 {ref64!r}, clip_grad_norm_ {ref32!r}")
    assert abs(got - ref64) <= 2.0 ** -22 * ref64
    # torch's own value is an fp32 norm of fp32 per-tensor norms: a few more roundings of 2^-24 each
    assert abs(got - ref32) <= (2.0 ** -22 + 8 * 2.0 ** -24) * ref64
    # the EMA state dict has the module's keys and differs from the live weights
    sd = opt.ema_state_dict(net, 0)
    assert set(sd) == set(net.state_dict()) and not torch.equal(sd["0.weight"], net.state_dict()["0.weight"])
    # a stock optimizer takes exactly the old path: no found_inf key
    sgd = torch.optim.SGD(list(frozen.parameters()), lr=0.0)
    info = train_step(list(frozen.parameters()), sgd, lambda: torch.nn.functional.mse_loss(frozen(x), y), max_grad_norm=0.5)
    assert "found_inf" not in info and set(info) == {"loss", "grad_norm", "collectives"}
