"""The structured-latent flow stage (trellis/models/structured_latent_flow.py on csrc/spconv.hip) against its torch compositions.  GPU only.

Released shapes: resolution 64, model_channels 1024, 16 heads, 24 blocks, io_block_channels [128], condition 1374 x 1024, one sample on a 64^3
spherical shell -- shell(64, 24, 26): 15 968 voxels (the fine set), and the cells of the 32^3 grid they fall into (the coarse set).

  1. every distinct convolution shape of the model -- 128 -> 128, 2048 -> 128, 256 -> 128 on the fine set, 128 -> 1024 and 1024 -> 1024 on the
     coarse set -- against the torch composition of the same operation in the operand type:
     27 x (index_select -> F.linear -> index_add_) over per-tap index lists built beforehand.  FLOP/s count existing neighbours only.
  2. one model forward, HIP operators against the torch operator set (tests/slat_flow_ref.py::TorchOps with the matrix work in the operand
     type, as a user would write it), and a 12-step guided sample (cfg 3.0 inside t in [0.5, 1], rescale_t 3.0).
The sides alternate in one process, GVF_ROUNDS times, device events around GVF_STEPS calls; min .. max over the rounds.
GVF_BENCH_SECTIONS (default "conv,model") selects the sections; GVF_BENCH_BLOCKS (default 24) the transformer blocks."""
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gvfdiffusion_amd import sparse as sp  # noqa: E402
from gvfdiffusion_amd.ops import spconv  # noqa: E402
from gvfdiffusion_amd.trellis.models import SLatFlowModel  # noqa: E402
from gvfdiffusion_amd.trellis.pipelines import FlowEulerSampler, sample_slat  # noqa: E402
import slat_flow_ref as R  # noqa: E402
import spconv_ref as S  # noqa: E402

dev = torch.device("cuda:0")
N_STEPS = int(os.environ.get("GVF_STEPS", 10))
ROUNDS = int(os.environ.get("GVF_ROUNDS", 3))
SECTIONS = set(os.environ.get("GVF_BENCH_SECTIONS", "conv,model").split(","))
BLOCKS = int(os.environ.get("GVF_BENCH_BLOCKS", 24))
DT = torch.float16


def timed(fn, n):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def alternate(sides, n=N_STEPS):
    out = {k: [] for k in sides}
    for _ in range(ROUNDS):
        for k, fn in sides.items():
            out[k].append(timed(fn, n))
    return out


def report(title, res, base="torch", flops=None):
    print(title)
    for k, v in res.items():
        ratio = "" if k == base else f"   torch / this = {min(res[base]) / min(v):.2f} x"
        rate = "" if flops is None else f"   {flops / min(v) / 1e9:.1f} TFLOP/s"
        print(f"    {k:<10s} {min(v):.3f} .. {max(v):.3f} ms{rate}{ratio}", flush=True)


def tap_lists(nbr):
    """Per tap: (rows that have the neighbour, the neighbours' rows) -- the torch composition's index lists."""
    out = []
    for k in range(27):
        rows = torch.nonzero(nbr[:, k] >= 0)[:, 0]
        out.append((rows, nbr[rows, k].long()))
    return out


def torch_conv(x, taps, w, bias):
    """27 x (index_select -> F.linear -> index_add_) in x's type; w [Cout, 27, Cin]."""
    out = bias.to(x.dtype).repeat(x.shape[0], 1)
    for k, (rows, src) in enumerate(taps):
        if rows.numel():
            out.index_add_(0, rows, F.linear(x.index_select(0, src), w[:, k]))
    return out


class TorchLpOps(R.TorchOps):
    """tests/slat_flow_ref.py::TorchOps with the matrix work done in the operand type on the device (F.linear, the 27-tap composition,
    scaled_dot_product_attention per sample): the torch route a user would write.  LayerNorm, modulation and the residual stream stay fp32."""

    def __init__(self, lp):
        super().__init__(lp)
        self._taps, self._w = {}, {}

    def _lpw(self, p):
        hit = self._w.get(id(p))
        if hit is None:
            hit = self._w[id(p)] = p.detach().to(self.lp)
        return hit

    def neighbor_map(self, coords):
        return spconv.build_neighbor_map(coords)            # the map is not what this baseline measures

    def linear(self, a16, lin, kind="f32"):
        y = F.linear(a16, self._lpw(lin.weight), None if lin.bias is None else self._lpw(lin.bias))
        if kind == "f32":
            return y.float()
        return F.gelu(y, approximate="tanh") if kind == "gelu" else y

    def linear_resid(self, x, a16, lin, gate=None):
        y = F.linear(a16, self._lpw(lin.weight), None if lin.bias is None else self._lpw(lin.bias)).float()
        x += y if gate is None else gate[None, :] * y
        return x

    def conv3(self, a16, nbr, conv, addend=None):
        key = nbr.data_ptr()
        if key not in self._taps:
            self._taps[key] = tap_lists(nbr)
        c = conv.conv
        y = torch_conv(a16, self._taps[key], self._lpw(c.weight).reshape(c.out_channels, 27, c.in_channels), c.bias.detach()).float()
        return y if addend is None else y + addend

    def attention(self, q, k, v, cu_q, cu_k, max_q, max_k, heads, gq=None, gk=None):
        Tq, C = q.shape
        d = C // heads
        qh, kh, vh = (t.reshape(t.shape[0], heads, d) for t in (q, k, v))
        if gq is not None:
            qh = (F.normalize(qh.float(), dim=-1) * gq * d ** 0.5).to(self.lp)
            kh = (F.normalize(kh.float(), dim=-1) * gk * d ** 0.5).to(self.lp)
        bq, bk = cu_q.tolist(), cu_k.tolist()
        outs = []
        for i in range(len(bq) - 1):
            qs, ks, vs = (t.permute(1, 0, 2)[None] for t in (qh[bq[i]:bq[i + 1]], kh[bk[i]:bk[i + 1]], vh[bk[i]:bk[i + 1]]))
            outs.append(F.scaled_dot_product_attention(qs, ks, vs)[0].permute(1, 0, 2))
        return torch.cat(outs).reshape(Tq, C)


def conv_section(fine, coarse):
    g = torch.Generator(device=dev).manual_seed(0)
    for name, coords, cin, cout in (("128 -> 128, fine", fine, 128, 128), ("2048 -> 128, fine", fine, 2048, 128), ("256 -> 128, fine", fine, 256, 128),
                                    ("128 -> 1024, coarse", coarse, 128, 1024), ("1024 -> 1024, coarse", coarse, 1024, 1024)):
        T = coords.shape[0]
        nbr = spconv.build_neighbor_map(coords)
        taps = tap_lists(nbr)
        x = torch.randn((T, cin), generator=g, device=dev).to(DT)
        w = torch.randn((cout, 3, 3, 3, cin), generator=g, device=dev) / (13.5 * cin) ** 0.5
        bias = torch.randn((cout,), generator=g, device=dev)
        wimg, w16 = spconv.pack_weight(w, DT), w.to(DT).reshape(cout, 27, cin)
        flops = S.flops_present(nbr, cin, cout)
        a, b = spconv.conv3(x, nbr, wimg, cout, bias=bias), torch_conv(x, taps, w16, bias)
        err = float((a - b.float()).abs().max() / b.float().abs().max())
        res = alternate({"torch": lambda: torch_conv(x, taps, w16, bias), "hip": lambda: spconv.conv3(x, nbr, wimg, cout, bias=bias)})
        report(f"conv3 {name}: T = {T}, {float((nbr >= 0).sum()) / T:.1f} neighbours per row, {flops / 1e9:.1f} GFLOP on existing neighbours "
               f"(hip vs torch: {err:.1e} of the largest output)", res, flops=flops)
    t = alternate({"torch": lambda: None, "hip": lambda: spconv.build_neighbor_map(fine)})
    print(f"neighbour map, T = {fine.shape[0]}: {min(t['hip']):.3f} .. {max(t['hip']):.3f} ms (built once per resolution)")


def model_section(fine):
    torch.manual_seed(0)
    cfg = dict(R.RELEASED, num_blocks=BLOCKS)
    with torch.device(dev):
        model = SLatFlowModel(**cfg).eval()
        for p in model.parameters():                     # the zero-initialised tensors too: a trained model has none
            if float(p.abs().max()) == 0:
                torch.nn.init.normal_(p, std=0.02)
    g = torch.Generator(device=dev).manual_seed(1)
    T = fine.shape[0]
    noise = torch.randn((T, 8), generator=g, device=dev)
    cond = torch.randn((1, 1374, 1024), generator=g, device=dev)
    neg = torch.zeros_like(cond)
    t = torch.tensor([600.0], device=dev)
    x = sp.SparseTensor(noise, fine)
    base = TorchLpOps(DT)
    a, b = model(x, t, cond).feats, model(x, t, cond, ops=base).feats
    print(f"model forward, {BLOCKS} blocks, T = {T}: hip vs torch operators {float((a - b).abs().max() / b.abs().max()):.1e} of the largest output")
    report(f"model forward ({DT})", alternate({"torch": lambda: model(x, t, cond, ops=base), "hip": lambda: model(x, t, cond)}, n=max(1, N_STEPS // 5)))
    params = dict(steps=12, cfg_strength=3.0, cfg_interval=(0.5, 1.0), rescale_t=3.0)
    norm = dict(mean=[0.0] * 8, std=[1.0] * 8)
    res = alternate({"torch": lambda: sample_slat(model, cond, neg, fine, params, norm, noise=noise, ops=base),
                     "hip": lambda: sample_slat(model, cond, neg, fine, params, norm, noise=noise)}, n=1)
    calls = sum(1 + (0.5 <= s <= 1.0) for s in FlowEulerSampler.timesteps(12, 3.0)[:-1])
    report(f"12-step guided sample ({calls} model calls)", res)


if __name__ == "__main__":
    t0 = time.time()
    fine = S.shell(64, 24, 26).to(dev)
    coarse = sp.SparseDownsample(2)(sp.SparseTensor(torch.zeros((fine.shape[0], 1), device=dev), fine)).coords.contiguous()
    print(f"{torch.cuda.get_device_name(0)}; shell(64, 24, 26): {fine.shape[0]} voxels, {coarse.shape[0]} after the downsampling; {DT}; "
          f"{ROUNDS} rounds of {N_STEPS} calls")
    if "conv" in SECTIONS:
        conv_section(fine, coarse)
    if "model" in SECTIONS:
        model_section(fine)
    print(f"({time.time() - t0:.0f} s)")
