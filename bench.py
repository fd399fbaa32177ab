#!/usr/bin/env python
"""bench.py -- the driver's benchmark contract for the 4D render-and-denoise hot path.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A "step" = one pass of the hot path over one batch of synthetic input: rendering ONE 4D sample
(24 frames, 800x800, 262 144 Gaussians with per-frame deltas, SH degree 2 -- BASELINE.json
configs[1]) through the fused batched rasteriser (gvf_rast_forward_batched).  Inputs are resident in
HBM when the timed region starts.  With N > 1 each rank renders its own sample (batch sharded over
the GPUs, weak scaling) and the ranks exchange the finished uint8 frames with ONE all-gather per
step (RCCL), overlapped with the next step's rendering on a side stream.
rank 0 prints ONE JSON line.  A plain run sets up, warms up, times the K steps and prints the headline figure; --full adds
the serial instrumented pass (stage times, `roofline`), the secondary workloads (differentiable render, DiT, end to end, live render,
sharded sampling) and the CPU baselines.
"""
import argparse
import ctypes
import json
import os
import sys
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")    # this pool's host driver does dmabuf IPC only: RCCL across processes needs it (set before HIP starts)
ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s spec peak
STAGES = ["order", "preprocess", "scan", "bin", "sort", "tile_sort", "blend"]


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gaussians", type=int, default=262_144)
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--sh-degree", type=int, default=2)
    ap.add_argument("--full", action="store_true",
                    help="besides the timed steps: the serial instrumented pass (stage times, roofline), the secondary workloads and the CPU baselines")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-dit", action="store_true", help="with --full: skip the secondary workloads")
    ap.add_argument("--e2e-only", action="store_true", help="profiling aid: run only the end-to-end leg and print its object")
    ap.add_argument("--dit-only", action="store_true", help="profiling aid: run only the DiT leg and print its object")
    ap.add_argument("--live-only", action="store_true", help="profiling aid: run only the live-render leg (32 x 128 x 512^2) and print its object")
    ap.add_argument("--streams", type=int, default=int(os.environ.get("GVF_BENCH_STREAMS", "2")),
                    help="4D samples kept in flight by the timed loop, one HIP stream + workspace + output buffer each (1 = strictly serial)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (rank 0's sample) as DIR/<name>.npy, for comparing two builds")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    return a


DUMP_MAX_ELEMS = 1 << 23          # 32 MB of float32 per dumped array: the whole dump stays under 64 MB


def dump_outputs(out_dir, color, num_rendered):
    """What a caller of gvf_rast_forward_batched receives for one step: the frames (F, 3, S, S) fp32 and the per-frame instance counts.
    Frames larger than DUMP_MAX_ELEMS are written as a fixed seeded sample of their elements (flat indices drawn with replacement, ascending), so that
    two builds run with the same arguments can be compared element for element."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    flat = color.reshape(-1)
    if flat.numel() <= DUMP_MAX_ELEMS:
        np.save(os.path.join(out_dir, "color.npy"), color.cpu().numpy().astype(np.float32))
    else:
        idx = torch.randint(flat.numel(), (DUMP_MAX_ELEMS,), generator=torch.Generator().manual_seed(0)).sort().values
        np.save(os.path.join(out_dir, "color_sample.npy"), flat[idx.to(flat.device)].cpu().numpy().astype(np.float32))
    np.save(os.path.join(out_dir, "num_rendered.npy"), num_rendered.cpu().numpy().astype(np.float64))


def _morton_perm(xyz, bits=5):
    """Stable argsort of the 3 x `bits`-bit Morton codes of positions in [-0.5, 0.5)^3 (GVF_BENCH_PRESORT)."""
    q = ((xyz + 0.5).clamp(0, 1 - 1e-6) * (1 << bits)).long()
    code = torch.zeros(xyz.shape[0], dtype=torch.long)
    for b in range(bits):
        for a in range(3):
            code |= ((q[:, a] >> b) & 1) << (3 * b + a)
    return torch.argsort(code, stable=True)


class RasterWorkload:
    """One 4D sample resident on the device + a preallocated workspace; step() enqueues one
    gvf_rast_forward_batched() on the current stream (no host sync)."""

    def __init__(self, dev, P, S, F, deg, seed):
        from gvfdiffusion_amd import synthetic, _lib, rasterizer as R
        camera_block = synthetic.camera_block
        self._lib, self.R, self.dev = _lib, R, dev
        self.P, self.S, self.F, self.deg, self.M = P, S, F, deg, (deg + 1) ** 2
        self.attrs = synthetic.random_gaussians(P, sh_degree=deg, seed=seed, scale_lo=0.002, scale_hi=0.01)
        self.delta_cpu = synthetic.random_deltas(F, P, seed=seed + 1)
        if os.environ.get("GVF_BENCH_PRESORT", "0") == "1":
            # measurement aid (NOT the default workload): the same sample with its Gaussians stored in Morton order of their positions, as a
            # caller who sorts a model once per sample would hand it over
            perm = _morton_perm(self.attrs["means3D"])
            self.attrs = {k: v[perm].contiguous() for k, v in self.attrs.items()}
            self.delta_cpu = self.delta_cpu[:, perm].contiguous()
        self.gm = synthetic.gaussian_model_from(self.attrs, deg, dev)
        self.delta = self.delta_cpu.to(dev)
        self.cams = [camera_block(azi=15.0 * f) for f in range(F)]
        self.frames = (_lib.GvfRastFrame * F)(*[
            R.make_frame(c["viewmatrix"], c["projmatrix"], c["campos"], c["tanfovx"], c["tanfovy"], f)
            for f, c in enumerate(self.cams)])
        # GVF_BIN_ALGO=1 benchmarks the radix binning instead of the default bucket binning (include/gvf_rast.h)
        self.st = R.make_settings(S, S, deg, _lib.RAST_MODE_MIP, synthetic.KERNEL_2D, 1.0, synthetic.BG,
                                  bin_algo=int(os.environ.get("GVF_BIN_ALGO", "0")))
        self.act = self.gm.activation_struct()
        g = self.gm
        self.raw = [t.contiguous().float() for t in (g._xyz, g.get_features, g._scaling, g._rotation, g._opacity.reshape(-1))]
        self.color = torch.empty((F, 3, S, S), dtype=torch.float32, device=dev)
        self.nr = torch.zeros((F,), dtype=torch.int32, device=dev)
        # size the workspace from one synchronised call
        out = R.rasterize_batched(self.st, list(self.frames), self.act, *self.raw, delta=self.delta)
        self.D_binned = int(out["num_rendered"].to(torch.int64).sum())       # instances the HIP path bins (alpha-box culled)
        self.cap = int(self.D_binned * 1.02) + 4096
        # D of the algorithm as the reference runs it (every tile of the 3-sigma rect): the roofline's algorithmic
        # bytes are priced on THIS count, not on the smaller one the HIP path gets away with
        st_up = R.make_settings(S, S, deg, _lib.RAST_MODE_MIP, synthetic.KERNEL_2D, 1.0, synthetic.BG, upstream_binning=True)
        out = R.rasterize_batched(st_up, list(self.frames), self.act, *self.raw, delta=self.delta)
        self.D = int(out["num_rendered"].to(torch.int64).sum())
        self.ws_bytes = R.workspace_bytes(P, F, S, S, self.cap)
        R._WORKSPACES.clear()
        del out
        torch.cuda.empty_cache()
        self.ws = torch.empty(self.ws_bytes + 256, dtype=torch.uint8, device=dev)
        self.ws_base = (self.ws.data_ptr() + 255) // 256 * 256

    def step(self):
        L, p = self._lib, self._lib.ptr
        rc = L.lib().gvf_rast_forward_batched(
            ctypes.byref(self.st), self.frames, self.F, ctypes.byref(self.act), self.P, self.M, p(self.raw[0]),
            p(self.raw[1]), p(self.raw[2]), p(self.raw[3]), p(self.raw[4]), p(self.delta), self.F,
            ctypes.c_void_p(self.ws_base), self.ws_bytes, self.cap, p(self.color), None, None, None, p(self.nr),
            L.current_stream(self.dev))
        L.check(rc, "gvf_rast_forward_batched")

    # algorithmic HBM bytes, SURVEY.md section 8d: B_alg/frame = P*P_in + D*24 + D*36 + H*W*4*3
    def alg_bytes_frame(self):
        p_in = 12 + 12 + 16 + 4 + 12 * self.M + 56          # xyz+scale+rot+op+sh (+ the 14-float delta row)
        d = self.D / self.F
        return self.P * p_in + d * 24 + d * 36 + self.S * self.S * 4 * 3

    def alg_bytes_blend_launch(self):
        # the blend launch covers all F frames.  SURVEY.md section 8d: 36 B fetched per (splat, tile) instance (xy 8 + conic / opacity 16 +
        # rgb 12) + the image (12 B per pixel).  (The 4-byte id the kernel also reads per instance is implementation traffic: not credited.)
        return self.D * 36 + self.F * self.S * self.S * 4 * 3


MFMA_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA peak


class DiTWorkload:
    """BASELINE configs[2]: configs/diffusion.yml DiT, batch 1, T=24, 32-step DPM-Solver++(2M) sampling on
    synthetic latents + random DINOv2-shaped conditions; weights seed-generated (no checkpoint here)."""

    def __init__(self, dev, T=24, seed=0, guidance=(1.0, 1.0), input_seed=None, dtype=None, weights="seed"):
        import json
        from gvfdiffusion_amd import synthetic
        from gvfdiffusion_amd.model.dit import DiT
        from gvfdiffusion_amd.model.dpmsolver import NoiseScheduleVP, model_wrapper, DPM_Solver
        from gvfdiffusion_amd.model.gaussian_diffusion import create_gaussian_diffusion
        man = json.load(open(os.path.join(ROOT, "tests", "golden", "dit_manifest.json")))
        self.cfg = man["config"]
        model = DiT(**self.cfg)
        # weights="trained_like": QK-RMSNorm gains in [0.5, 3], cross-attention scores with a std of ~7 octaves, and (below) conditions with a
        # few high-norm context tokens >= 30 octaves out -- the score statistics of a trained denoiser, hostile to a max-free softmax
        gen = synthetic.dit_state_dict_trained_like if weights == "trained_like" else synthetic.dit_state_dict
        model.load_state_dict(gen(man["state_dict"], seed=seed), strict=True)
        # operand type of the matrix pipe: None = the module's own rule (configs/diffusion.yml use_fp16: true -> fp16, the reference's
        # accelerate precision; GVF_DIT_DTYPE overrides), "bf16" / "fp16" = explicit
        model.set_compute_dtype(dtype)
        self.model = model.to(dev).eval().enable_graph(os.environ.get("GVF_DIT_GRAPH", "1") == "1")
        self.model.count_attention_fallbacks(True)      # (an atomic per workgroup that LEAVES the fast path; nothing on the fast path)
        self.dtype_name = {torch.float16: "fp16", torch.bfloat16: "bf16"}[self.model._lp()]
        gen_in = synthetic.dit_inputs_hostile if weights == "trained_like" else synthetic.dit_inputs
        # input_seed: one seed = one sample (B = 1); a list = that many DIFFERENT samples stacked into one batch (each generated exactly as its
        # B = 1 twin, so a batched run can be compared with the single-sample runs bit for bit)
        seeds = list(input_seed) if isinstance(input_seed, (list, tuple)) else [seed + 1 if input_seed is None else input_seed]
        parts = [gen_in(B=1, T=T, seed=s_) for s_ in seeds]
        inp = {k: torch.cat([p_[k] for p_ in parts]).to(dev) for k in parts[0]}
        self.x = inp.pop("x"); self.t_golden = inp.pop("t")
        self.is_golden_case = weights == "seed" and seed == 0 and seeds == [1] and T == 24        # = tests/golden/dit_full_golden.npz's inputs
        self.cond = inp
        uncond = dict(inp); uncond["cond_images"] = torch.zeros_like(inp["cond_images"])
        ns = NoiseScheduleVP("discrete", betas=torch.from_numpy(create_gaussian_diffusion(noise_schedule="cosine", predict_type="v").betas))
        mf = model_wrapper(self.model, ns, model_type="v", model_kwargs={}, guidance_type="classifier-free",
                           guidance_scale=guidance[0], guidance_scale2=guidance[1], condition=inp, unconditional_condition=uncond)
        self.solver = DPM_Solver(mf, ns, algorithm_type="dpmsolver++")
        self.T = T

    def sample(self, steps=32):
        return self.solver.sample(self.x, steps=steps, t_start=1.0, t_end=1 / 1000, order=2, skip_type="time_uniform",
                                  method="multistep")

    def parity_vs_fp32_golden(self):
        """rel-L2 of ONE forward of this model (this operand type) against the reference's own fp32 output of the same weights and inputs
        (tests/golden/dit_full_golden.npz: model/dit.py imported and run by tests/golden/make_golden.py; data, not the oracle) -- the figure
        tests/test_dit_fp16_gpu.py::test_full_config_forward_matches_reference_golden asserts, put into the driver's line."""
        import numpy as np
        assert self.is_golden_case
        gold = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "dit_full_golden.npz"))["y"]).to(self.x.device)
        with torch.no_grad():
            y = self.model(self.x, self.t_golden, **self.cond)
        return float((y.double() - gold.double()).norm() / gold.double().norm())

    def flops_per_nfe(self, hoisted):
        """2MNK per Linear, 4 Lq Lk C per attention, configs/diffusion.yml at B=1."""
        T, N, C, Li, Ls, nb = self.T, 512, 512, 1370, 4096, 12
        M = T * N
        lin = lambda m, n, k: 2.0 * m * n * k
        att = lambda b, lq, lk: 4.0 * b * lq * lk * C
        per_block = (lin(M, 3 * C, C) + att(T, N, N) + lin(M, C, C)             # spatial self
                     + lin(M, 3 * C, C) + att(N, T, T) + lin(M, C, C)           # temporal self
                     + lin(M, C, C) + att(T, N, Li) + lin(M, C, C)              # image cross (q, attn, out)
                     + lin(M, C, C) + att(T, N, Ls) + lin(M, C, C)              # static cross
                     + lin(M, 4 * C, C) + lin(M, C, 4 * C))                     # mlp
        ctx_block = lin(T * Li, 2 * C, C) + lin(T * Ls, 2 * C, C)               # to_kv(context) as written (per frame)
        small = lin(M, C, 16) + lin(M, 16, C)
        ctx_once = lin(T * Li, C, 1024) + lin(T * Ls, C, 14)
        return nb * per_block + small + (0.0 if hoisted else nb * ctx_block + ctx_once)


def bench_dit(dev, nfe=32):
    nfe = int(os.environ.get("GVF_BENCH_DIT_NFE", nfe))

    def timed(w_):
        w_.sample(steps=4)                  # warm-up: weight conversion, condition cache, allocator, graph capture
        w_.sample(steps=nfe)                # ... and one untimed pass of the timed workload (per-job state: the modulation table of this time grid)
        torch.cuda.synchronize()
        w_.model.attention_fallbacks()      # (reset)
        t0_ = time.perf_counter()
        w_.sample(steps=nfe)                # exactly nfe network evaluations
        torch.cuda.synchronize()
        dt_ = time.perf_counter() - t0_
        w_.fallback_wgs = w_.model.attention_fallbacks()      # tiled-attention workgroups of the timed pass that re-ran on the exact softmax path
        return dt_

    def guard_fields(w_):
        per_nfe = w_.model.attention_workgroups(w_.x.shape[0], w_.T, 512)
        return {"fallback_wgs": w_.fallback_wgs, "attention_wgs": per_nfe * nfe, "fallback_frac": round(w_.fallback_wgs / (per_nfe * nfe), 5)}
    # GVF_BENCH_DIT_BATCH=B (measurement aid, --dit-only): the same step on a batch of B different samples in ONE forward; the line then carries
    # ms_per_sample_forward beside ms_per_nfe and skips the B = 1 extras
    batch = int(os.environ.get("GVF_BENCH_DIT_BATCH", "1"))
    if batch > 1:
        wb = DiTWorkload(dev, input_seed=list(range(1, batch + 1)))
        db = timed(wb)
        return {"metric": f"DiT denoise step, batch {batch} in one forward (measurement aid)", "batch": batch, "dtype": wb.dtype_name, "nfe": nfe,
                "ms_per_nfe": round(db / nfe * 1e3, 3), "ms_per_sample_forward": round(db / nfe / batch * 1e3, 3),
                "value": round(batch * nfe / db, 3), "unit": "sample-steps/s"}
    w = DiTWorkload(dev)
    dt = timed(w)
    per = dt / nfe
    guards = guard_fields(w)
    # parity in the driver's line: the full-config output of ONE forward against the reference's fp32 golden, both operand
    # types, beside the reference's own autocast error of the same type (tests/golden/dit_autocast_golden.npz); taken AFTER the timed pass
    import numpy as np
    auto = np.load(os.path.join(ROOT, "tests", "golden", "dit_autocast_golden.npz"))
    parity = {"what": "rel-L2 of one full-config forward (configs/diffusion.yml, B=1, T=24) vs the reference's own fp32 output "
                      "(tests/golden/dit_full_golden.npz); north_star's 1e-4 is below one ulp of either operand type (DESIGN.md 3.1b) -- the bar "
                      "the tests hold is the reference's own autocast error of the same type",
              w.dtype_name: round(w.parity_vs_fp32_golden(), 7),
              "reference_autocast": {k_: round(float(auto[f"full_rel_l2_{k_}"]), 7) for k_ in ("fp16", "bf16")}}
    # the same step on "trained-like" weights and hostile conditions (synthetic.dit_state_dict_trained_like / dit_inputs_hostile): what the
    # max-free softmax's range guard (and fp16's shift) cost when the scores look like a trained model's; both operand types
    hostile = None
    if os.environ.get("GVF_BENCH_DIT_HOSTILE", "1") == "1":
        hostile = {}
        for dt_name in ("fp16", "bf16"):
            wh = DiTWorkload(dev, dtype=dt_name, weights="trained_like")
            dh = timed(wh)
            hostile[dt_name] = dict({"value": round(nfe / dh, 3), "unit": "steps/s", "ms_per_nfe": round(dh / nfe * 1e3, 3)}, **guard_fields(wh))
            del wh
            torch.cuda.empty_cache()
        import inspect
        from gvfdiffusion_amd import synthetic
        kw_w = {k_: v_.default for k_, v_ in inspect.signature(synthetic.dit_state_dict_trained_like).parameters.items() if v_.default is not inspect.Parameter.empty}
        kw_i = {k_: v_.default for k_, v_ in inspect.signature(synthetic.dit_inputs_hostile).parameters.items() if v_.default is not inspect.Parameter.empty}
        # (the generators' ACTUAL parameters, read off their signatures: ADVICE r5 -- the note used to advertise harsher values than were run)
        hostile["generator"] = {"dit_state_dict_trained_like": {k_: kw_w[k_] for k_ in ("gamma_lo", "gamma_hi", "cross_gain", "outlier_gain")},
                                "dit_inputs_hostile": {"token_gain": kw_i["token_gain"]}}
        hostile["note"] = (f"QK-RMSNorm gains U[{kw_w['gamma_lo']}, {kw_w['gamma_hi']}], cross-attention to_q / to_kv(k) x {kw_w['cross_gain']} + a rank-one "
                           f"heavy-tail term x {kw_w['outlier_gain']}, three high-norm context tokens per context (x {kw_i['token_gain']}); parity on this model: "
                           "tests/test_dit_fp16_gpu.py::test_full_config_trained_like_weights")
    fh, fa = w.flops_per_nfe(True), w.flops_per_nfe(False)
    dtype_name = w.dtype_name
    # the same step with the other 16-bit operand type (same kernels, same MFMA rate): BASELINE.json names bf16, the reference runs fp16
    other = None
    if os.environ.get("GVF_BENCH_DIT_OTHER_DTYPE", "1") == "1":
        wo = DiTWorkload(dev, dtype="bf16" if dtype_name == "fp16" else "fp16")
        do = timed(wo)
        parity[wo.dtype_name] = round(wo.parity_vs_fp32_golden(), 7)
        other = {"dtype": wo.dtype_name, "value": round(nfe / do, 3), "unit": "steps/s", "ms_per_nfe": round(do / nfe * 1e3, 3),
                 "frac": round(fh / (do / nfe) / 1e12 / MFMA_PEAK_TFLOPS, 5)}
        del wo
        torch.cuda.empty_cache()
    # two independent samples in flight (own DiT instance, stream and Python thread each; gvfdiffusion_amd.utils.run_in_flight): the
    # serving-style throughput of the same B = 1 step.  Secondary figure: `value` / `ms_per_nfe` / `roofline` stay those of ONE sample.
    flight = None
    if os.environ.get("GVF_BENCH_DIT_INFLIGHT", "1") == "1":
        from gvfdiffusion_amd.utils import run_in_flight
        w2 = DiTWorkload(dev, input_seed=7)
        ref = [w.sample(steps=4), w2.sample(steps=4)]                  # serial warm-up / reference of both instances
        jobs = [lambda slot, ww=ww: ww.sample(steps=4) for ww in (w, w2)]
        run_in_flight(jobs, dev, 2)                                      # warm the side streams' allocator pools
        got = run_in_flight(jobs, dev, 2)
        assert all(torch.equal(a_, b_) for a_, b_ in zip(got, ref)), "in-flight sampling changed the latents"
        jobs = [lambda slot, ww=ww: ww.sample(steps=nfe) for ww in (w, w2)]
        w2.sample(steps=nfe)                                             # (per-job state of the second instance: its modulation table)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_in_flight(jobs, dev, 2)
        torch.cuda.synchronize()
        d2 = time.perf_counter() - t0
        flight = {"samples_in_flight": 2, "value": round(2 * nfe / d2, 3), "unit": "steps/s (both samples)",
                  "ms_per_solver_step": round(d2 / nfe * 1e3, 3), "achieved_TFLOPs": round(2 * fh * nfe / d2 / 1e12, 2),
                  "frac": round(2 * fh * nfe / d2 / 1e12 / MFMA_PEAK_TFLOPS, 5),
                  "note": "two independent B=1 samplers on two HIP streams (two DiT instances, same weights): latents identical to the "
                          "serial runs; three in flight measured lower (scripts/dit_two_streams.py)"}
        del w2
    cfg3 = None
    if os.environ.get("GVF_BENCH_DIT_CFG3", "1") == "1":
        # the same solver with two-scale classifier-free guidance on: one solver step = ONE forward of batch 3
        # (full-uncond | uncond | cond, model/dpmsolver.py:318-340) -- what a guided sampling run pays per step
        del w
        torch.cuda.empty_cache()
        w3 = DiTWorkload(dev, guidance=(3.0, 1.5))
        w3.sample(steps=4)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        w3.sample(steps=16)
        torch.cuda.synchronize()
        d3 = (time.perf_counter() - t0) / 16
        cfg3 = {"ms_per_solver_step": round(d3 * 1e3, 3), "ms_per_sample_forward": round(d3 * 1e3 / 3, 3),
                "achieved_TFLOPs": round(3 * fh / d3 / 1e12, 2), "frac": round(3 * fh / d3 / 1e12 / MFMA_PEAK_TFLOPS, 5),
                "note": "guidance_scale 3.0 / 1.5: batch-3 forward per step; fixed per-launch costs amortised over 3 samples"}
    return {"metric": "DiT denoise steps/sec (B=1, T=24, configs/diffusion.yml, 32-step DPM-Solver++ multistep)",
            "cfg3": cfg3, "in_flight": flight, "softmax_guard": guards, "trained_like_weights": hostile, "parity_vs_fp32_golden": parity,
            "value": round(nfe / dt, 3), "unit": "steps/s", "ms_per_nfe": round(per * 1e3, 3), "nfe": nfe, "dtype": dtype_name,
            "dtype_note": "operand type of the MFMA contractions (fp32 accumulation, stream, LayerNorm, softmax): fp16 = what the reference "
                          "runs (accelerate mixed_precision='fp16'; configs/diffusion.yml use_fp16: true), 3.4e-4 of the fp32 reference output "
                          "against 2.8e-3 for bf16 (tests/test_dit_fp16_gpu.py); `other_dtype` = the same step with BASELINE.json's bf16",
            "other_dtype": other,
            "roofline": {"bound": "mfma", "unit": "TFLOP/s", "peak": MFMA_PEAK_TFLOPS,
                         "achieved": round(fh / per / 1e12, 2), "frac": round(fh / per / 1e12 / MFMA_PEAK_TFLOPS, 5),
                         "flops_per_nfe_hoisted": fh, "flops_per_nfe_as_written": fa,
                         "note": "achieved counts only the per-step work actually executed (condition K/V hoisted out of "
                                 "the loop); as-written equivalent = %.2f TFLOP/s" % (fa / per / 1e12)}}


class E2EWorkload:
    """The inference_dpm_latent.py chain at the named shapes (BASELINE configs[3] / [4]): DPM-Solver over the DiT
    (configs/diffusion.yml, B=1) -> de-normalise -> motion-VAE decode of P static Gaussians x T frames (released VAE
    config) -> batched render of the T frames (SH degree 0, mip filter, per-frame 14-channel deltas).  Random-init weights
    of the released architectures, synthetic conditions; `sample_seed` picks the sample (its noise and conditions)."""

    def __init__(self, dev, P=262_144, S=800, T=24, sample_seed=0):
        """sample_seed: one seed = one sample per chain() (B = 1); a list = that many DIFFERENT samples whose sampling runs as ONE batched
        DPM-Solver call on one DiT (decode + render then sample by sample) -- what a rank of the sharded job does with its share."""
        import json
        from gvfdiffusion_amd import synthetic
        from gvfdiffusion_amd.model.autoencoder import GSKLTemporalVariationalAutoEncoder
        from gvfdiffusion_amd.renderers import GaussianRenderer
        self.dev, self.P, self.S, self.T = dev, P, S, T
        self.seeds = list(sample_seed) if isinstance(sample_seed, (list, tuple)) else [sample_seed]
        self.batched = isinstance(sample_seed, (list, tuple))
        self.w = DiTWorkload(dev, T=T, input_seed=[1 + s_ for s_ in self.seeds] if self.batched else 1 + sample_seed)
        self.calls = {"n": 0}
        inner = self.w.solver.model

        def counted(x, t):
            self.calls["n"] += 1
            return inner(x, t)
        self.w.solver.model = counted
        man = json.load(open(os.path.join(ROOT, "tests", "golden", "vae_manifest.json")))
        torch.manual_seed(0)
        vae = GSKLTemporalVariationalAutoEncoder(**man["config"], num_timesteps=T)
        with torch.no_grad():
            for p in vae.parameters():
                p.copy_(torch.randn_like(p) * (1.0 / p.shape[1] ** 0.5 if p.dim() == 2 else 0.05))
            vae.to_outputs.weight.mul_(0.02)            # deltas of a few per cent of the object size, as a trained decoder gives
        self.vae = vae.to(dev).set_compute_dtype(self.w.model._lp())      # the chain runs in ONE 16-bit operand type (the reference: fp16 autocast)
        self.gms, self.queries_all = [], []
        for s_ in self.seeds:
            attrs = synthetic.random_gaussians(P, sh_degree=0, seed=s_)
            gm = synthetic.gaussian_model_from(attrs, 0, dev)
            self.gms.append(gm)
            self.queries_all.append(torch.cat([gm._xyz, gm._features_dc.reshape(P, 3), gm._scaling, gm._rotation, gm._opacity], 1)[None].float())
        self.gm, self.queries = self.gms[0], self.queries_all[0]
        self.rend = GaussianRenderer({"resolution": S, "near": synthetic.NEAR, "far": synthetic.FAR, "ssaa": 1, "bg_color": (1, 1, 1)})
        self.rend.pipe.use_mip_gaussian = True
        self.rend.pipe.kernel_size = synthetic.KERNEL_2D
        self.ext = torch.stack([synthetic.orbit_w2c(360.0 * f / T, 15.0) for f in range(T)]).to(dev)
        self.K = synthetic.intrinsics().to(dev)

    def chain(self, method="adaptive", steps=100, fresh_conditions=True):
        """-> ([ms sample, ms decode, ms render], NFE count, rendered frames) -- of the ONE sample, or (batched) summed over / a list for the batch.
        fresh_conditions (round 6): the sample arrives with NEW condition tensors (clones: same values, other objects), as every sample of a job
        does, so its step-invariant condition products (condition projections, 24 K / V caches: ~4.7 ms) are computed INSIDE the timed sampling
        stage; rounds 1-5 timed a second chain on the warm-up's tensors, whose products were cached."""
        T, S = self.T, self.S
        nb = len(self.seeds)
        if fresh_conditions:
            for k_ in list(self.w.cond):
                self.w.cond[k_] = self.w.cond[k_].clone()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 + 2 * nb)]
        self.calls["n"] = 0
        ev[0].record()
        x = self.w.solver.sample(self.w.x, steps=steps, t_start=1.0, t_end=1 / 1000, order=2, skip_type="time_uniform", method=method)
        ev[1].record()
        outs = []
        for j in range(nb):
            lat = (x[j:j + 1] * 1.5 + 0.02).reshape(T, x.shape[2], x.shape[3])
            delta = self.vae.decode(lat, self.queries_all[j]).float()
            ev[2 + 2 * j].record()
            outs.append(self.rend.render_frames(self.gms[j], self.ext, self.K, delta_pc=delta[0].contiguous(), sync=False))
            ev[3 + 2 * j].record()
        torch.cuda.current_stream().synchronize()      # this chain's stream only: another sample may be in flight on its own
        assert all(o.rgb.shape == (T, 3, S, S) for o in outs)
        # NFE as the solver reports it (the reference's count: `order` evaluations per attempted adaptive step); the evaluations actually run can
        # differ by a few (a rejected step keeps its first evaluation; a speculated one is dropped): self.calls["n"]
        nfe = self.w.solver.last_nfe if method == "adaptive" and self.w.solver.last_nfe is not None else self.calls["n"]
        ms = [ev[0].elapsed_time(ev[1]), sum(ev[1 + 2 * j].elapsed_time(ev[2 + 2 * j]) for j in range(nb)),
              sum(ev[2 + 2 * j].elapsed_time(ev[3 + 2 * j]) for j in range(nb))]
        return ms, nfe, (outs if self.batched else outs[0])


def bench_e2e(dev, P=262_144, S=800, T=24):
    """BASELINE configs[3] on one MI355X: adaptive DPM-Solver (steps=100 as the script's --rescale_timesteps default).
    Secondary figure, not part of `value`."""
    import contextlib
    e = E2EWorkload(dev, P, S, T)
    with torch.no_grad(), contextlib.redirect_stdout(sys.stderr):     # the solver reports its NFE on stdout, as upstream does
        e.chain()                                    # warm-up: weight conversion, graph capture, workspace
        # three samples (each on fresh condition tensors), the MEDIAN one reported: a single chain is 37 host round trips and moved by +-3 %
        # from run to run on one box (profiles/r06_prepare_conditions.txt, the full-bench A/B); all three walls are in the line
        runs = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stages, nfe, out = e.chain()
            runs.append((time.perf_counter() - t0, stages, nfe, e.calls["n"]))
            assert bool(torch.isfinite(out.rgb).all())
        wall, (ms_sample, ms_decode, ms_render), nfe, model_calls = sorted(runs, key=lambda r: r[0])[1]
    return {"metric": "end-to-end 4D sample (adaptive DPM-Solver -> VAE decode -> 24-frame render), BASELINE configs[3]",
            "value": round(T / wall, 2), "unit": "frames/s", "wall_ms": round(wall * 1e3, 2), "wall_ms_of_3_samples": [round(r[0] * 1e3, 2) for r in runs],
            "nfe": nfe, "model_calls": model_calls,
            "adaptive_steps": dict(getattr(e.w.solver, "spec_stats", {})),
            "stage_ms": {"sample": round(ms_sample, 2), "vae_decode": round(ms_decode, 2), "render": round(ms_render, 2)},
            "config": {"gaussians": P, "resolution": S, "frames": T, "sampler": "dpmsolver++ adaptive, steps=100, order 2",
                       "dtype": f"{e.w.dtype_name} models (DiT and motion VAE), f32 rasteriser"}}


def bench_live_render(dev, P=262_144, T=32, V=128, S=512):
    """The reference's LIVE render job of one sample (utils/inference_utils.py:240-269): 32 timesteps x 128 orbit cameras
    = 4096 frames of 512 x 512, SH degree 0, mip filter, per-timestep 14-channel deltas, frames leave as uint8 -- through the product's
    batched driver gvfdiffusion_amd.utils.render_sample_frames (96-frame launches, two in flight).  Secondary figure, not part of `value`."""
    from gvfdiffusion_amd import synthetic
    from gvfdiffusion_amd.renderers import GaussianRenderer
    from gvfdiffusion_amd.utils import orbit_cameras, render_sample_frames
    attrs = synthetic.random_gaussians(P, sh_degree=0, seed=7)
    g = torch.Generator().manual_seed(11)
    delta = torch.randn((T, P, 14), generator=g) * 0.01
    if os.environ.get("GVF_BENCH_PRESORT", "0") == "1":          # measurement aid, see RasterWorkload
        perm = _morton_perm(attrs["means3D"])
        attrs = {k: v[perm].contiguous() for k, v in attrs.items()}
        delta = delta[:, perm].contiguous()
    delta = delta.to(dev)
    gm = synthetic.gaussian_model_from(attrs, 0, dev)
    rend = GaussianRenderer({"resolution": S, "near": synthetic.NEAR, "far": synthetic.FAR, "ssaa": 1, "bg_color": (1, 1, 1)})
    rend.pipe.kernel_size = synthetic.KERNEL_2D
    K, cams = synthetic.intrinsics().to(dev), orbit_cameras(V).to(dev)

    chunk, n_streams = int(os.environ.get("GVF_LIVE_CHUNK", "96")), int(os.environ.get("GVF_LIVE_STREAMS", "2"))   # (the driver's defaults)

    def job():
        n, acc = 0, 0
        for _, frames in render_sample_frames(rend, gm, delta, K, extrinsics=cams, chunk_frames=chunk, streams=n_streams):
            n += frames.shape[0]
            acc += int(frames[0, 0, 0, 0])        # (touch each chunk on the host, as a consumer that writes PNGs would)
        return n

    with torch.no_grad():
        job()                                      # warm-up: workspace sizing
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = job()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    assert n == T * V
    return {"metric": "the reference's live render job: one sample = 32 timesteps x 128 orbit cameras x 512x512, SH degree 0, uint8 frames "
                      "(utils/inference_utils.py:240-269) through render_sample_frames",
            "value": round(n / dt, 1), "unit": "frames/s", "ms_per_sample": round(dt * 1e3, 2), "frames": n, "gaussians": P, "resolution": S,
            "chunk_frames": chunk, "chunks_in_flight": n_streams}


class _OneRank:
    """torch.distributed's few calls used by bench_sharded_sampling, for a job of ONE rank without a process group (the default N = 1 line's
    configs[4] anchor): nothing to wait for, nothing to exchange."""
    @staticmethod
    def barrier(): pass
    @staticmethod
    def get_backend(): return "none (one rank, no process group)"
    @staticmethod
    def get_world_size(): return 1
    @staticmethod
    def all_gather(out, t): out[0].copy_(t)
    @staticmethod
    def all_reduce(t, op=None): pass
    class ReduceOp:
        MAX = None


def bench_sharded_sampling(dev, dist, rank, world, P, S, T, total_batch=8, steps=32, mode=None):
    """BASELINE configs[4]: batch-sharded sampling (inference_dpm_latent.py:168-273 processes its batch sample by sample with no
    cross-sample operation).  Rank r owns samples r, r + world, ... of a batch of `total_batch`: 32-step DPM-Solver++(2M) on the
    DiT -> VAE decode -> 24-frame render, uint8 frames, then the ONE collective of the path: an all-gather of every rank's
    frames (RCCL over xGMI).  Reported: whole-job samples / frames / denoise steps per second from the max-over-ranks wall
    time, the slowest rank's per-NFE time, and the gather on its own.
    mode "batched" (default): a rank's samples are sampled as ONE batch on one DiT (the multistep solver is batch-transparent; every launch of
    the forward covers the whole batch), then decoded and rendered one by one: 1.04-1.05 x the serial job on the boxes measured with the
    full-length warm-up (profiles/r06_sharded_modes.txt).  "inflight" (rounds 3-5): B = 1 chains, two in flight on two streams and two host
    threads (two DiT instances): 0.98-1.04 x, the spread follows the box's host cores.  "batched_inflight": two batches in flight, the
    slowest.  GVF_BENCH_SHARD_MODE selects; the N = 1 line reports the first two.  dist=None: one rank, no process group."""
    import contextlib
    from gvfdiffusion_amd import distributed as D, rasterizer as R
    dist = _OneRank if dist is None else dist
    mode = mode or os.environ.get("GVF_BENCH_SHARD_MODE", "batched")
    total = max(total_batch, world)                     # every rank owns at least one sample
    mine = D.shard_indices(total, rank, world)
    b_loc = len(mine)
    timings = []
    if mode in ("batched", "batched_inflight"):
        # "batched_inflight": the rank's share as TWO batches in flight (own DiT instance, stream and host thread each): the batch amortises the
        # per-launch costs, the second stream fills the other's tails and the decode / render of one batch runs under the sampling of the other
        n_fl = 2 if (mode == "batched_inflight" and b_loc >= 2) else 1
        per = (b_loc + n_fl - 1) // n_fl
        es = [E2EWorkload(dev, P, S, T, sample_seed=[rank + 1000 * k for k in range(g * per, min(b_loc, (g + 1) * per))]) for g in range(n_fl)]

        def batch_chain(idx, slot=0):
            """this slot's samples `idx`: one batched sampling call -> per-sample decode -> render -> uint8 frames"""
            with torch.no_grad():
                res = es[slot].chain(method="multistep", steps=steps)
                timings.append((res[0], res[1] * len(idx)))              # (one evaluation of the batch = one NFE per sample)
                return [R.frames_to_uint8(o.rgb) for o in res[2]]
        run = lambda: D.sample_decode_render_sharded(None, total, device=dev, gather=False, batch_chain=batch_chain, in_flight=n_fl)
    else:
        # a rank with several samples keeps two of them in flight (own models, stream and thread each: gvfdiffusion_amd.utils.run_in_flight)
        n_fl = 2 if b_loc >= 2 and os.environ.get("GVF_BENCH_DIT_INFLIGHT", "1") == "1" else 1
        es = [E2EWorkload(dev, P, S, T, sample_seed=rank + 1000 * k) for k in range(n_fl)]

        def chain(slot, i):
            """sample i: 32-step sampling -> decode -> render -> uint8 frames (the chain of inference_dpm_latent.py:225-272)"""
            with torch.no_grad():
                res = es[slot].chain(method="multistep", steps=steps)
                timings.append((res[0], res[1]))
                return R.frames_to_uint8(res[2].rgb)
        run = lambda: D.sample_decode_render_sharded(chain, total, device=dev, in_flight=n_fl, gather=False)

    with torch.no_grad(), contextlib.redirect_stdout(sys.stderr):
        for e_ in es:
            # warm-up, serially, with the TIMED step count: weight conversion, condition caches, and the per-job state of this time grid -- the
            # modulation table of its 33 times and the hipGraph captured against that table (bench_dit's timed() does the same).  A 4-step
            # warm-up left both inside the timed region: ~2 extra eager forwards + 12 ms per DiT instance, i.e. 90 ms of a batch-8 job's 1.4 s
            # and the reason the first batched figures of this round read 8 % slower than the B = 1 ones.
            e_.chain(method="multistep", steps=steps)
        timings.clear()
        dist.barrier(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        local, _ = run()
        g0, g1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        g0.record()
        gathered = D.gather_frames(local, total)            # the path's one collective (RCCL over xGMI)
        g1.record()
        dist.barrier(); torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    assert gathered.shape == (total, T, 3, S, S) and torch.equal(gathered[rank::world], local)
    ms_sample = sum(t_[0][0] for t_ in timings); ms_decode = sum(t_[0][1] for t_ in timings); ms_render = sum(t_[0][2] for t_ in timings)
    nfe = sum(t_[1] for t_ in timings)
    t = torch.tensor([dt, ms_sample / max(nfe, 1), g0.elapsed_time(g1)], dtype=torch.float64, device=dev if not str(dist.get_backend()).startswith("gloo") else "cpu")
    every = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(every, t)                           # per-rank record: wall, ms per NFE, gather ms
    per_rank = [[float(v) for v in e.tolist()] for e in every]
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt, ms_nfe, ms_gather = (float(v) for v in t.tolist())
    n_samples = total
    fh, es_dtype = es[0].w.flops_per_nfe(True), es[0].w.dtype_name
    del es
    torch.cuda.empty_cache()
    return {"metric": "batch-sharded sampling (BASELINE configs[4]): 32-step DPM-Solver++ on the DiT -> VAE decode -> 24-frame "
                      "800x800 render per sample, one frame all-gather at the end",
            "mode": mode + {"batched": ": a rank's samples are sampled as ONE batch on one DiT, decoded and rendered one by one",
                            "batched_inflight": ": a rank's samples as TWO batches in flight (two DiT instances, two streams), each sampled as one batch",
                            }.get(mode, ": B = 1 chains, two in flight on two streams (two DiT instances)"),
            "samples": n_samples, "samples_per_rank": b_loc, "samples_in_flight_per_rank": b_loc if mode.startswith("batched") else n_fl,
            "dit_batch_per_forward": (b_loc + n_fl - 1) // n_fl if mode.startswith("batched") else 1, "streams_per_rank": n_fl, "wall_ms": round(dt * 1e3, 2),
            "samples_per_s": round(n_samples / dt, 3), "frames_per_s": round(n_samples * T / dt, 2),
            "denoise_steps_per_s": round(n_samples * steps / dt, 2), "ms_per_nfe_slowest_rank": round(ms_nfe, 3),
            "gather_ms": round(ms_gather, 3), "gather_us": round(ms_gather * 1e3, 1), "gather_bytes_per_rank": int(local.numel()),
            "gather_bytes_total": int(gathered.numel()),
            # the functional record of the N > 1 path: who took part, over what, and every rank's own figures (rank order)
            "rccl_ranks": int(dist.get_world_size()), "backend": str(dist.get_backend()),
            "per_rank": {"wall_ms": [round(r_[0] * 1e3, 2) for r_ in per_rank], "ms_per_nfe": [round(r_[1], 3) for r_ in per_rank],
                         "gather_us": [round(r_[2] * 1e3, 1) for r_ in per_rank]},
            "rank0_stage_ms_per_sample": {"sample": round(ms_sample / b_loc, 2), "vae_decode": round(ms_decode / b_loc, 2),
                                          "render": round(ms_render / b_loc, 2)},
            # per GPU, from the wall time of the whole chain (decode, render and gather included): a lower bound on the DiT's own fraction
            "dit_roofline_frac": round(fh * b_loc * steps / dt / 1e12 / MFMA_PEAK_TFLOPS, 5),
            "ms_per_nfe_per_gpu_throughput": round(dt * 1e3 / (b_loc * steps), 3),
            "dtype": es_dtype, "scaling": "weak" if world <= total_batch else "replicas"}


def bench_backward(dev, attrs, S, deg, iters=8):
    """The operator as a training step sees it (train_vae.py:321-352): one frame per call under autograd, forward +
    backward, same Gaussians / resolution as the headline workload.  Secondary figure, not part of `value`."""
    from gvfdiffusion_amd import synthetic
    from gvfdiffusion_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from gvfdiffusion_amd.synthetic import camera_block
    leaves = {k: v.to(dev).requires_grad_(True) for k, v in attrs.items()}
    P = leaves["means3D"].shape[0]
    w = torch.randn((3, S, S), device=dev)
    cams = [camera_block(azi=15.0 * f) for f in range(4)]

    def one(i):
        c = cams[i % 4]
        rast = GaussianRasterizer(GaussianRasterizationSettings(
            image_height=S, image_width=S, tanfovx=c["tanfovx"], tanfovy=c["tanfovy"], kernel_size=synthetic.KERNEL_2D,
            subpixel_offset=None, bg=torch.tensor(synthetic.BG, device=dev), scale_modifier=1.0, viewmatrix=c["viewmatrix"].to(dev),
            projmatrix=c["projmatrix"].to(dev), sh_degree=deg, campos=c["campos"].to(dev), prefiltered=False, debug=False))
        color, _ = rast(means3D=leaves["means3D"], means2D=torch.zeros((P, 3), device=dev), shs=leaves["shs"], colors_precomp=None,
                        opacities=leaves["opacities"], scales=leaves["scales"], rotations=leaves["rotations"], cov3D_precomp=None)
        (color * w).sum().backward()

    for i in range(3):
        one(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        one(i)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / iters * 1e3
    return {"metric": "differentiable render, forward + backward, one frame per call (incl. the host sync on num_rendered)",
            "ms_per_frame": round(ms, 3), "frames_per_s": round(1e3 / ms, 1), "gaussians": P, "resolution": S, "sh_degree": deg}


def pmc_traffic(kernel, a, S, F):
    """(bytes, note): HBM-side bytes per launch of `kernel` from the newest committed PMC summary (the counters cannot be
    collected from inside the benchmark process).  None unless the summary was taken on THIS workload and on THESE kernel
    sources (profiles/*_pmc_raster.json carries gvfdiffusion_amd._build.raster_source_hash() of the build it profiled)."""
    import glob
    from gvfdiffusion_amd._build import raster_source_hash
    if (a.gaussians, S, F, a.sh_degree) != (262144, 800, 24, 2):
        return None, "not the profiled workload"
    files = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "*_pmc_raster.json")))
    if not files:
        return None, "no PMC summary committed"
    doc = json.load(open(files[-1]))
    if doc.get("raster_source_hash") != raster_source_hash():
        return None, f"stale: {os.path.basename(files[-1])} was collected on other rasteriser sources (re-run scripts/gpu_pmc.sh)"
    kernels = doc["kernels"]
    k = kernels.get(kernel) or next((v for n, v in kernels.items() if n.startswith(kernel + "<")), None)   # template instance
    return (None, "kernel not in the summary") if k is None else (int(k["traffic_bytes_per_launch"]), os.path.basename(files[-1]))


def pmc_valu_issue(kernel, a, S, F):
    """VALU-issue roofline of a compute-bound kernel from the committed SQ-counter summary (profiles/*_pmc_raster_sq.json,
    same source-hash stamp): SQ_ACTIVE_INST_VALU / SQ_BUSY_CYCLES-normalised issue fraction.  None when absent or stale."""
    import glob
    from gvfdiffusion_amd._build import raster_source_hash
    if (a.gaussians, S, F, a.sh_degree) != (262144, 800, 24, 2):
        return None
    files = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "*_pmc_raster_sq.json")))
    if not files:
        return None
    doc = json.load(open(files[-1]))
    if doc.get("raster_source_hash") != raster_source_hash():
        return None
    k = doc["kernels"].get(kernel) or next((v for n, v in doc["kernels"].items() if n.startswith(kernel + "<")), None)
    return None if k is None else dict(k, source=os.path.basename(files[-1]))


def cpu_baseline(work, budget_s=12.0):
    """The CPU oracle (kind "port": the reference has no CPU Gaussian rasteriser)
    timed on this box's host cores on the first frames of the same sample."""
    import oracle
    n = lambda t: t.detach().cpu().numpy()
    g = work.gm
    raw = [n(t) for t in (g._xyz, g.get_features, g._scaling, g._rotation, g._opacity)]
    from rast_util import oracle_render
    done, t0 = 0, time.time()
    while done < work.F:
        oa = oracle.gaussian_activate(*raw, n(work.delta_cpu[done]), aabb=[-0.5, -0.5, -0.5, 1, 1, 1],
                                      scale_bias=float(g.scale_bias), opacity_bias=float(g.opacity_bias),
                                      min_kernel_size=float(g.mininum_kernel_size), scaling_activation=1)
        attrs = {k: torch.from_numpy(oa[k]) for k in ("means3D", "scales", "rotations", "shs")}
        attrs["opacities"] = torch.from_numpy(oa["opacities"])
        oracle_render(oracle, attrs, work.cams[done], work.S, work.S, work.deg, mode=0)
        done += 1
        if time.time() - t0 > budget_s:
            break
    dt = time.time() - t0
    return {"value": round(done / dt, 4), "unit": "frames/s", "cores": oracle.num_threads(), "kind": "port",
            "sample": f"first {done} of the {work.F} frames of the same sample (activations + full render) in {dt:.1f} s; "
                      "reference has no CPU Gaussian path (renderers/pytorch_renderer is CUDA-only Strivec)"}


def dit_cpu_baseline(T_sample=24, T=24):
    """The DiT leg's CPU figure: the fp32 torch restatement of the reference's DiT._forward (oracle/dit_ref.py, pinned to the
    reference by tests/test_oracle_dit.py; kind "port") on this box's host cores: ONE whole network evaluation of the same
    model and conditions (all T frames -- the temporal attention couples them, so nothing is extrapolated)."""
    import json
    from gvfdiffusion_amd import synthetic
    from oracle import dit_ref
    man = json.load(open(os.path.join(ROOT, "tests", "golden", "dit_manifest.json")))
    sd = synthetic.dit_state_dict(man["state_dict"], seed=0)
    inp = synthetic.dit_inputs(B=1, T=T_sample, seed=1)
    with torch.no_grad():
        t0 = time.time()
        y = dit_ref.dit_forward(sd, man["config"], inp["x"], inp["t"], inp["cond_images"], inp["static_latent"],
                                inp["deformation_position_xyz"], precision="fp32")
        dt = time.time() - t0
    assert bool(torch.isfinite(y).all())
    return {"value": round(1.0 / (dt * T / T_sample), 5), "unit": "steps/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"one full forward of the same DiT (all {T_sample} frames, one NFE) in {dt:.1f} s "
                      "(torch fp32 restatement of model/dit.py:449-480)"}


def main():
    a = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback)")
    dev = torch.device("cuda", local % torch.cuda.device_count())      # (several ranks on one GPU only with GVF_BENCH_BACKEND=gloo: a test aid)
    torch.cuda.set_device(dev)
    dist = None
    # GVF_BENCH_FORCE_DIST=1: take the N > 1 code path (RCCL init, frame all-gather on the side stream, reductions) with a
    # single rank -- the only way to execute it on a one-GPU box
    multi = world > 1 or os.environ.get("GVF_BENCH_FORCE_DIST") == "1"
    if multi:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        for k_, v_ in (("MASTER_PORT", "29533"), ("RANK", "0"), ("WORLD_SIZE", "1"), ("LOCAL_RANK", "0")):
            os.environ.setdefault(k_, v_)          # GVF_BENCH_FORCE_DIST=1 without a launcher
        # the image exports NCCL_DEBUG=VERSION and RCCL printf()s its banner to stdout when the communicator is created:
        # point fd 1 at stderr while that happens, so that stdout carries the one JSON line only
        sys.stdout.flush()
        saved = os.dup(1)
        os.dup2(2, 1)
        try:
            backend = os.environ.get("GVF_BENCH_BACKEND", "nccl")       # "nccl" = RCCL over xGMI; "gloo": the N > 1 code path on a one-GPU box
            if backend == "nccl":
                dist.init_process_group("nccl", device_id=dev)
            else:
                dist.init_process_group(backend)
            warm = torch.zeros(1, device=dev if backend == "nccl" else "cpu")
            dist.all_reduce(warm)                      # forces communicator creation now
            torch.cuda.synchronize()
        finally:
            sys.stdout.flush()
            ctypes.CDLL(None).fflush(None)         # the banner sits in the C library's stdio buffer: push it out while fd 1 still is stderr
            os.dup2(saved, 1)
            os.close(saved)

    if a.dit_only:
        print(json.dumps(bench_dit(dev)))
        return
    if a.live_only:
        print(json.dumps(bench_live_render(dev, a.gaussians)))
        return
    if a.e2e_only:
        print(json.dumps(bench_e2e(dev, a.gaussians, a.res, a.frames)))
        return
    from gvfdiffusion_amd import _lib
    work = RasterWorkload(dev, a.gaussians, a.res, a.frames, a.sh_degree, seed=rank)
    F, S = a.frames, a.res

    # Consecutive 4D samples are independent, so the timed loop keeps `--streams` of them in flight, each on its own HIP stream with
    # its own workspace and frame buffer (what gvfdiffusion_amd.utils.render_sample_frames does with consecutive frame chunks): the
    # HBM-bound front of one sample (projection, binning) runs under the VALU-bound compositing of the other.  Stage times and the
    # roofline object come from a strictly serial, instrumented pass over the same K steps first.
    # Every slot in flight holds its OWN sample (different Gaussians and deltas: seed + 1000 slot), as consecutive samples of a job do.
    from gvfdiffusion_amd import distributed as D
    n_slots = max(1, a.streams)
    slots = [work] + [RasterWorkload(dev, a.gaussians, a.res, a.frames, a.sh_degree, seed=rank + 1000 * k) for k in range(1, n_slots)]
    rstreams = [torch.cuda.Stream(device=dev) for _ in range(n_slots)]

    # Frame exchange (N > 1), BASELINE's "all-gather over xGMI only for the final frame collection": the job this loop measures is `steps`
    # batches of `world` samples, one per rank per step, and EVERY sample that `value` counts is collected inside the timed region: its
    # frames are converted to uint8 (46 MB per sample) and all-gathered on a side stream while the next step renders (one
    # all_gather_into_tensor per step; the closing barrier + synchronize waits for the last one).  GVF_BENCH_GATHER_EVERY_STEP=0 is the
    # render-only variant (ONE gather of the last step's frames at the end) and says so in config.collective.
    every_step = multi and os.environ.get("GVF_BENCH_GATHER_EVERY_STEP", "1") == "1"
    side = torch.cuda.Stream(device=dev) if every_step else None
    nbuf = max(2, n_slots)
    u8 = [torch.empty((F, 3, S, S), dtype=torch.uint8, device=dev) for _ in range(nbuf)] if multi else None
    gathered = [torch.empty((world * F, 3, S, S), dtype=torch.uint8, device=dev) for _ in range(nbuf)] if every_step else None
    ready = [torch.cuda.Event() for _ in range(nbuf)] if every_step else None
    consumed = [torch.cuda.Event() for _ in range(nbuf)] if every_step else None

    def final_gather(n_active, n_steps):
        """The job's one collective: every rank's last finished sample, (world, F, 3, S, S) uint8 on every rank."""
        if not multi or every_step:
            return None
        k = (n_steps - 1) % n_active
        torch.cuda.current_stream().wait_stream(rstreams[k])
        work.R.frames_to_uint8(slots[k].color, out=u8[0])
        return D.gather_frames(u8[0][None], total=world)

    def step(i, n_active):
        k = i % n_active
        with torch.cuda.stream(rstreams[k]):
            slots[k].step()
            if every_step:
                b = i % nbuf
                rstreams[k].wait_event(consumed[b])                            # buffer b free again
                work.R.frames_to_uint8(slots[k].color, out=u8[b])
                ready[b].record()
                with torch.cuda.stream(side):
                    side.wait_event(ready[b])
                    if dist.get_backend() == "nccl":
                        dist.all_gather_into_tensor(gathered[b], u8[b])
                    else:                          # gloo test aid (ranks sharing one GPU box): gather_frames stages through the host
                        gathered[b].copy_(D.gather_frames(u8[b][None], total=world).view_as(gathered[b]))
                    consumed[b].record(side)

    def barrier():
        if multi:
            dist.barrier()
        torch.cuda.synchronize()

    if every_step:
        for e in consumed:
            e.record()
    # ---- pass 1 (--full): serial and instrumented (per-stage HIP events inside the library): stage times, roofline, single-stream step time
    if a.full:
        for i in range(a.warmup):
            step(i, 1)
        final_gather(1, max(a.warmup, 1))           # first all-gather of the process: RCCL sets its channels up here, outside any timed region
        barrier()
        _lib.check(_lib.lib().gvf_rast_profile_enable(1), "profile_enable")
        t0 = time.perf_counter()
        for i in range(a.steps):
            step(i, 1)
        final_gather(1, a.steps)
        barrier()
        dt_serial = time.perf_counter() - t0
        ms = (ctypes.c_float * len(STAGES))()
        calls = ctypes.c_int(0)
        _lib.check(_lib.lib().gvf_rast_profile_read(ms, ctypes.byref(calls)), "profile_read")
        _lib.lib().gvf_rast_profile_enable(0)
    # ---- pass 2: the timed K steps, n_slots samples in flight (every slot warmed at least twice, whatever W is)
    serial_frames = []
    for k in range(n_slots):                    # what each slot's sample looks like rendered alone, on one stream
        with torch.cuda.stream(rstreams[k]):
            slots[k].step()
        rstreams[k].synchronize()
        serial_frames.append(slots[k].color.clone())
        slots[k].color.zero_()
    for i in range(max(a.warmup, 2 * n_slots)):
        step(i, n_slots)
    final_gather(n_slots, max(a.warmup, 2 * n_slots))      # (warms the communicator's all-gather path too)
    barrier()
    t0 = time.perf_counter()
    for i in range(a.steps):
        step(i, n_slots)
    got = final_gather(n_slots, a.steps)
    barrier()
    dt = time.perf_counter() - t0
    for k in range(n_slots):
        assert torch.equal(slots[k].color, serial_frames[k]), f"slot {k}: frames rendered with {n_slots} samples in flight differ from the serial render"
    assert n_slots < 2 or not torch.equal(serial_frames[0], serial_frames[1]), "the slots must hold different samples"
    if got is not None:
        k = (a.steps - 1) % n_slots
        assert got.shape == (world, F, 3, S, S) and torch.equal(got[rank], work.R.frames_to_uint8(slots[k].color))
    if every_step:                               # the last gathered batch holds this rank's last sample at its rank-major position
        b, k = (a.steps - 1) % nbuf, (a.steps - 1) % n_slots
        assert torch.equal(gathered[b].view(world, F, 3, S, S)[rank], work.R.frames_to_uint8(slots[k].color))
    if a.dump_outputs and rank == 0:              # the slot that rendered the last timed step
        k = (a.steps - 1) % n_slots
        dump_outputs(a.dump_outputs, slots[k].color, slots[k].nr)

    t = torch.tensor([dt, dt_serial if a.full else 0.0], dtype=torch.float64, device=dev if (not multi or dist.get_backend() == "nccl") else "cpu")
    if multi:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt, dt_serial = float(t[0].item()), float(t[1].item())

    # overflow check after the timed region (no sync inside it)
    assert all(int(w_.nr.to(torch.int64).sum()) <= w_.cap for w_ in slots), "workspace overflow during the timed region"

    if rank == 0:
        out = {
            "metric": "4D frames/sec (800x800x24f, 256k Gaussians) + DiT denoise steps/sec",
            "value": round(world * F * a.steps / dt, 2),
            "unit": "frames/s",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": round(dt / a.steps * 1e3, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": "BASELINE configs[1]: single-GPU HIP rasteriser, one 4D sample per step = "
                                   f"{F} frames x {S}x{S}, {a.gaussians} Gaussians + per-frame deltas (fused "
                                   f"activations), SH degree {a.sh_degree}, mip 2D filter, white bg",
                       "gaussians": a.gaussians, "resolution": S, "frames_per_step": F, "sh_degree": a.sh_degree,
                       "instances_per_frame": round(work.D / F, 1), "instances_binned_per_frame": round(work.D_binned / F, 1), "parallelism": f"sample-sharded x{world}",
                       "samples_in_flight": n_slots,
                       "pipelining": f"{n_slots} DIFFERENT samples in flight per GPU (own Gaussians, deltas, HIP stream, workspace and frame buffer "
                                     "each; every slot's frames are asserted bit-identical to its serial render); with --full, stage_ms_per_step, roofline "
                                     "and ms_per_step_serial come from a serial instrumented pass over the same steps",
                       "collective": None if not multi else (
                           "every counted sample is collected inside the timed region: uint8 conversion + one all_gather_into_tensor per step "
                           f"({world} x {F * 3 * S * S / 1e6:.0f} MB) on a side stream, overlapped with the next step's rendering" if every_step else
                           "RENDER-ONLY timing (GVF_BENCH_GATHER_EVERY_STEP=0): only the LAST step's frames are gathered (once, at the end of the "
                           "timed region); the other steps' frames are counted but not collected")},
        }
        if a.full:
            traffic, traffic_note = pmc_traffic("blend_kernel", a, S, F)
            valu_issue = pmc_valu_issue("blend_kernel", a, S, F)
            ncalls = max(1, calls.value)
            stage_ms = {s: ms[k] / ncalls for k, s in enumerate(STAGES)}
            blend_s = stage_ms["blend"] * 1e-3
            achieved = work.alg_bytes_blend_launch() / blend_s / 1e9 if blend_s > 0 else 0.0
            gpu_frame_s = sum(stage_ms.values()) * 1e-3 / F
            out.update({
                "ms_per_step_serial": round(dt_serial / a.steps * 1e3, 4),       # one sample at a time on one stream (with the stage events)
                "roofline": {"bound": "hbm", "kernel": "blend_kernel (R6, one launch = all frames of the step)",
                             "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": traffic,
                             "traffic_source": "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this workload (scripts/gpu_pmc.sh, "
                                               "scripts/pmc_summary.py; FETCH x2 gfx950 correction), bytes per launch, from the committed "
                                               "summary stamped with the rasteriser source hash: " + traffic_note,
                             # the same launch priced on the instances the kernel actually touches (alpha-box culled binning), 36 B each
                             "frac_on_binned_instances": round((work.D_binned * 36 + F * S * S * 12) / blend_s / 1e9 / HBM_PEAK_GBS, 5) if blend_s > 0 else 0,
                             "valu_issue": valu_issue,
                             # The bound that actually binds this launch: the compositing loop is 16 vector instructions per list
                             # entry of which one is a v_exp_f32; on the `valu_issue` scale (SQ_ACTIVE_INST_VALU x 2 cycles / busy cycles) that mix
                             # topped out at ~0.69 with the loop of rounds 5-6 (profiles/r05_blend_phase_stamps.txt) and at ~0.73 with the lane-mask form of
                             # its predicates (the loop-only figure 41.4 -> 38.9 ticks per entry per SIMD, same 16 vector instructions:
                             # profiles/r06_ubench_blend_step.txt); `achieved` = the counter figure of the committed SQ pass.
                             # The one restructuring not priced before round 6 -- exponents from six v_mfma_f32_4x4x1 per 4 splats, 11 vector
                             # instructions per entry -- is 8 % SLOWER in a loop-only micro-benchmark (profiles/r06_ubench_blend_step.txt), so the
                             # kernel stays and this is its roofline; the HBM figure above is what north_star asked to see.
                             "binding_bound": None if not valu_issue else {
                                 "bound": "valu", "unit": "fraction of VALU issue cycles", "achieved": valu_issue.get("valu_issue"), "peak": 0.73,
                                 "frac": round(valu_issue.get("valu_issue", 0.0) / 0.73, 4),
                                 "source": valu_issue.get("source")},
                             # BASELINE's north star prices "tile-sort + blend" together: the per-tile sort moves 8 B in + 4 B out per binned
                             # instance (PMC: 0.25 GB per launch = exactly that), priced like the blend on upstream's instance count
                             "tile_sort_plus_blend": (lambda b_, t_: {"alg_bytes": int(b_), "ms": round(t_ * 1e3, 4), "achieved_GBs": round(b_ / t_ / 1e9, 2),
                                                                      "frac": round(b_ / t_ / 1e9 / HBM_PEAK_GBS, 5)})(
                                 work.alg_bytes_blend_launch() + 12.0 * work.D, (stage_ms["blend"] + stage_ms["tile_sort"]) * 1e-3)
                             if stage_ms["blend"] + stage_ms["tile_sort"] > 0 else None,
                             "alg_bytes_per_launch": int(work.alg_bytes_blend_launch()),
                             "avg_launch_ms": round(stage_ms["blend"], 4)},
                "stage_ms_per_step": {k: round(v, 4) for k, v in stage_ms.items()},
                "pipeline_roofline": {"alg_bytes_per_frame": int(work.alg_bytes_frame()),
                                      "achieved_GBs": round(work.alg_bytes_frame() / gpu_frame_s / 1e9, 2) if gpu_frame_s else 0,
                                      "frac": round(work.alg_bytes_frame() / gpu_frame_s / 1e9 / HBM_PEAK_GBS, 5) if gpu_frame_s else 0},
            })
        if a.full and not multi and not a.no_dit:
            for w_ in slots:
                w_.__dict__.pop("ws", None)
            torch.cuda.empty_cache()
            out["differentiable_render"] = bench_backward(dev, work.attrs, a.res, a.sh_degree)
            out["dit"] = bench_dit(dev)
            torch.cuda.empty_cache()
            out["end_to_end"] = bench_e2e(dev, a.gaussians, a.res, a.frames)
            torch.cuda.empty_cache()
            out["live_render"] = bench_live_render(dev, a.gaussians)
            torch.cuda.empty_cache()
            if os.environ.get("GVF_BENCH_SHARDED_ANCHOR", "1") == "1":
                # BASELINE configs[4]'s anchor at N = 1: the sharded-sampling job with ONE rank -- batch 8, 32 steps,
                # decode + render + uint8 frames of every sample -- through the same code the N > 1 line runs (no process group: _OneRank).
                # `serial_B1_equivalent`: 8 x (32 x the B = 1 ms/NFE of this line's dit leg + the e2e leg's decode + render) for comparison.
                sh = bench_sharded_sampling(dev, None, 0, 1, a.gaussians, a.res, a.frames)
                if os.environ.get("GVF_BENCH_SHARD_COMPARE", "1") == "1":
                    keep = ("wall_ms", "samples_per_s", "denoise_steps_per_s", "ms_per_nfe_per_gpu_throughput", "rank0_stage_ms_per_sample",
                            "samples_in_flight_per_rank", "dit_batch_per_forward", "streams_per_rank")
                    # ("batched_inflight", two batches of 4 on two streams, is the slowest by far -- 1.5-2.8 s against 1.3-1.4 s: two persistent
                    # attention grids and two one-workgroup-per-CU row-block grids cannot share the chip -- and is left to GVF_BENCH_SHARD_MODE)
                    for name_, mode_ in (("two_B1_chains_in_flight", "inflight"),):
                        alt = bench_sharded_sampling(dev, None, 0, 1, a.gaussians, a.res, a.frames, mode=mode_)
                        sh[name_] = {k_: alt[k_] for k_ in keep}
                e2 = out["end_to_end"]["stage_ms"]
                ser_ms = sh["samples"] * (32 * out["dit"]["ms_per_nfe"] + e2["vae_decode"] + e2["render"])
                sh["serial_B1_equivalent"] = {"wall_ms": round(ser_ms, 2), "denoise_steps_per_s": round(sh["samples"] * 32 / ser_ms * 1e3, 2),
                                              "speedup_of_this_line": round(ser_ms / sh["wall_ms"], 4)}
                out["sharded_sampling"] = sh
        if a.full and multi and not a.no_dit:
            for w_ in slots:
                w_.__dict__.pop("ws", None)
            torch.cuda.empty_cache()
        if a.full and not multi and not a.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(work)
            if "dit" in out:
                out["dit"]["cpu_baseline"] = dit_cpu_baseline()
    if a.full and multi and not a.no_dit:
        # every rank takes part; rank 0 prints (the driver reads ONE JSON line)
        if rank != 0:
            for w_ in slots:
                w_.__dict__.pop("ws", None)
            torch.cuda.empty_cache()
        shard = bench_sharded_sampling(dev, dist, rank, world, a.gaussians, a.res, a.frames)
        if rank == 0:
            out["dit"] = {"metric": "DiT denoise steps/sec, whole job (sample-sharded, 32-step DPM-Solver++ multistep per sample)",
                          "value": shard["denoise_steps_per_s"], "unit": "steps/s", "ms_per_nfe": shard["ms_per_nfe_per_gpu_throughput"],
                          "ms_per_nfe_one_sample_latency": shard["ms_per_nfe_slowest_rank"], "samples_in_flight_per_rank": shard["samples_in_flight_per_rank"],
                          "dtype": shard["dtype"], "roofline": {"bound": "mfma", "unit": "TFLOP/s", "peak": MFMA_PEAK_TFLOPS,
                                                        "frac": shard["dit_roofline_frac"]}}
            out["end_to_end"] = shard
            out["rccl_ranks"], out["backend"] = shard["rccl_ranks"], shard["backend"]
            out["per_rank_ms_per_nfe"] = shard["per_rank"]["ms_per_nfe"]
            out["gather"] = {"bytes_per_rank": shard["gather_bytes_per_rank"], "bytes_total": shard["gather_bytes_total"], "us": shard["gather_us"],
                             "per_rank_us": shard["per_rank"]["gather_us"]}
    if rank == 0:
        print(json.dumps(out))
    if multi:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
