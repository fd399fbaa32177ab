"""The sparse-structure stage (trellis/models/sparse_structure_flow.py, sparse_structure_vae.py on csrc/conv3d.hip) against torch.  GPU only.

Released shapes (from memory of the public release): flow model resolution 16, patch 1, model_channels 1024, 16 heads, 24 blocks, condition
1374 x 1024; decoder latent 8, channels [512, 128, 32], two residual blocks per level, 16^3 -> 64^3.  One sample.

  1. every distinct convolution shape of the decoder -- 8 -> 512, 512 -> 512, 512 -> 1024 (shuffle2 store) at 16^3; 128 -> 128, 128 -> 256
     (shuffle2) at 32^3; 32 -> 32, 32 -> 1 at 64^3 -- against torch's F.conv3d (channels_last_3d, the operand type), and, at the four shapes
     gvf_spconv3 accepts, against the submanifold kernel on the full grid's neighbour map.
  2. the decoder, one flow forward, and a guided sample with the released sampler settings (from memory: 25 steps, cfg 7.5 inside t in
     [0.5, 1], rescale_t 3), HIP operators against the torch operator set with the matrix work in the operand type on the device.
The sides alternate in one process, GVF_ROUNDS times, device events around GVF_STEPS calls; min .. max over the rounds.
GVF_BENCH_SECTIONS (default "conv,stage") selects the sections; GVF_BENCH_BLOCKS (default 24) the transformer blocks."""
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from gvfdiffusion_amd.ops import conv3d, spconv  # noqa: E402
from gvfdiffusion_amd.trellis.models import SparseStructureDecoder, SparseStructureFlowModel  # noqa: E402
from gvfdiffusion_amd.trellis.pipelines import FlowEulerSampler, sample_sparse_structure  # noqa: E402
from bench_slat_flow import TorchLpOps, alternate, report, N_STEPS, ROUNDS, DT  # noqa: E402
import conv3d_ref as C  # noqa: E402
import sparse_structure_ref as R  # noqa: E402

dev = torch.device("cuda:0")
SECTIONS = set(os.environ.get("GVF_BENCH_SECTIONS", "conv,stage").split(","))
BLOCKS = int(os.environ.get("GVF_BENCH_BLOCKS", 24))
SAMPLER = dict(steps=25, cfg_strength=7.5, cfg_interval=(0.5, 1.0), rescale_t=3.0)


def dense_view(rows, grid):
    """(B X Y Z, C) rows -> the (B, C, X, Y, Z) channels_last_3d view of the same memory."""
    B, X, Y, Z = grid
    return rows.reshape(B, X, Y, Z, rows.shape[1]).permute(0, 4, 1, 2, 3)


class TorchDenseOps(TorchLpOps):
    """bench_slat_flow.TorchLpOps with the dense convolution as F.conv3d on the channels_last_3d view of the rows, in the operand type."""

    def dense_conv3(self, a16, grid, conv, addend=None, store="rows"):
        hit = self._w.get((id(conv.weight), "cl3d"))
        if hit is None:
            hit = self._w[(id(conv.weight), "cl3d")] = conv.weight.detach().to(self.lp).contiguous(memory_format=torch.channels_last_3d)
        y = F.conv3d(dense_view(a16[:, :conv.in_channels], grid), hit, self._lpw(conv.bias), padding=1)
        y = y.permute(0, 2, 3, 4, 1).reshape(-1, conv.out_channels).float()
        if store == "shuffle2":
            y = C.pixel_shuffle2(y, grid)
        return y if addend is None else y + addend

    @staticmethod
    def occupancy(logits, grid):
        return R.TorchOps.occupancy(logits, grid)


def full_grid(n):
    g = torch.arange(n, dtype=torch.int32, device=dev)
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    return torch.stack([torch.zeros_like(x), x, y, z], dim=-1).reshape(-1, 4).contiguous()


def conv_section():
    g = torch.Generator(device=dev).manual_seed(0)
    for n, cin, cout, store in ((16, 8, 512, "rows"), (16, 512, 512, "rows"), (16, 512, 1024, "shuffle2"), (32, 128, 128, "rows"),
                                (32, 128, 256, "shuffle2"), (64, 32, 32, "rows"), (64, 32, 1, "rows")):
        grid = (1, n, n, n)
        rows = n ** 3
        ld = max(64, cin)
        x = torch.zeros((rows, ld), device=dev, dtype=DT)
        x[:, :cin] = torch.randn((rows, cin), generator=g, device=dev).to(DT)
        w = torch.randn((cout, cin, 3, 3, 3), generator=g, device=dev) / (27 * cin) ** 0.5
        bias = torch.randn((cout,), generator=g, device=dev)
        wimg = conv3d.pack_weight(w, DT)
        wcl, b16 = w.to(DT).contiguous(memory_format=torch.channels_last_3d), bias.to(DT)
        xv = dense_view(x[:, :cin], grid)
        hip = lambda: conv3d.conv3(x, grid, wimg, cin, cout, bias=bias, store=store)
        tor = lambda: F.conv3d(xv, wcl, b16, padding=1)
        ref = tor().permute(0, 2, 3, 4, 1).reshape(rows, cout).float()
        ref = C.pixel_shuffle2(ref, grid) if store == "shuffle2" else ref
        err = float((hip() - ref).abs().max() / ref.abs().max())
        sides = {"torch": tor, "hip": hip}
        if cin % 64 == 0 and cout % 64 == 0:
            nbr = spconv.build_neighbor_map(full_grid(n))
            simg = spconv.pack_weight(w.permute(0, 2, 3, 4, 1).contiguous(), DT)
            sides["spconv3"] = lambda: spconv.conv3(x, nbr, simg, cout, bias=bias, cin=cin)
        flops = C.flops(grid, cin, cout)
        report(f"conv3d {cin} -> {cout} at {n}^3 ({store} store, fp32 out): {flops / 1e9:.1f} GFLOP incl. padding taps "
               f"(hip vs torch: {err:.1e} of the largest output)", alternate(sides), flops=flops)


def stage_section():
    torch.manual_seed(0)
    with torch.device(dev):
        flow = SparseStructureFlowModel(**dict(R.FLOW_RELEASED, num_blocks=BLOCKS)).eval()
        dec = SparseStructureDecoder(**R.DEC_RELEASED).eval()
        for m in (flow, dec):
            for p in m.parameters():                     # the zero-initialised tensors too: a trained model has none
                if float(p.abs().max()) == 0:
                    torch.nn.init.normal_(p, std=0.02)
    g = torch.Generator(device=dev).manual_seed(1)
    noise = torch.randn((1, 8, 16, 16, 16), generator=g, device=dev)
    cond = torch.randn((1, 1374, 1024), generator=g, device=dev)
    neg = torch.zeros_like(cond)
    t = torch.tensor([600.0], device=dev)
    base = TorchDenseOps(DT)
    z = C.to_rows(noise)
    grid = (1, 16, 16, 16)
    a, b = dec.forward_rows(z, grid)[0], dec.forward_rows(z, grid, base)[0]
    print(f"decoder 16^3 -> 64^3: hip vs torch operators {float((a - b).abs().max() / b.abs().max()):.1e} of the largest logit")
    report(f"decoder ({DT})", alternate({"torch": lambda: dec.forward_rows(z, grid, base), "hip": lambda: dec.forward_rows(z, grid)}, n=max(1, N_STEPS // 2)))
    logits = a.reshape(1, -1).contiguous()
    report("occupancy read-out, 64^3 (torch: argwhere)", alternate({"torch": lambda: base.occupancy(logits, (1, 64, 64, 64)),
                                                                    "hip": lambda: conv3d.occupancy_coords(logits, (1, 64, 64, 64))}))
    a, b = flow(noise, t, cond), flow(noise, t, cond, ops=base)
    print(f"flow forward, {BLOCKS} blocks, 4096 tokens: hip vs torch operators {float((a - b).abs().max() / b.abs().max()):.1e} of the largest output")
    report(f"flow forward ({DT})", alternate({"torch": lambda: flow(noise, t, cond, ops=base), "hip": lambda: flow(noise, t, cond)}, n=max(1, N_STEPS // 5)))
    res = alternate({"torch": lambda: sample_sparse_structure(flow, dec, cond, neg, 1, SAMPLER, noise=noise, ops=base),
                     "hip": lambda: sample_sparse_structure(flow, dec, cond, neg, 1, SAMPLER, noise=noise)}, n=1)
    calls = sum(1 + (0.5 <= s <= 1.0) for s in FlowEulerSampler.timesteps(SAMPLER["steps"], SAMPLER["rescale_t"])[:-1])
    report(f"25-step guided sample + decoder + coords ({calls} model calls)", res)


if __name__ == "__main__":
    t0 = time.time()
    print(f"{torch.cuda.get_device_name(0)}; {DT}; {ROUNDS} rounds of {N_STEPS} calls")
    if "conv" in SECTIONS:
        conv_section()
    if "stage" in SECTIONS:
        stage_section()
    print(f"({time.time() - t0:.0f} s)")
