/*
 * gvf_optim.h -- C ABI of the fused optimizer step of the training loop: everything the reference does after backward()
 * (train_vae.py:355-375, train_latent.py:209-225: GradScaler unscale + inf check, clip_grad_norm_ over all parameters, AdamW.step per
 * group, update_ema for every rate) as three launches over a fixed set of fp32 tensors.
 *
 * Tables (device memory, built once by the caller):
 *   tensors[T]   gvf_optim_tensor: the pointers of one tensor (p, g, m, v, up to 4 EMA copies) and its group index.
 *   chunks[n]    gvf_optim_chunk: {tensor, count, first}: elements [first, first + count) of that tensor.  `first` is a multiple of 4,
 *                count <= gvf_optim_chunk_len(), no chunk crosses a tensor, zero-element tensors have no chunk.
 *
 * gvf_optim_norm (two launches: per-chunk partials, then one workgroup):
 *   gu = g * inv_scale in fp32 (inv_scale: one device float, null = 1); gu^2 accumulated in double, one partial per chunk in the chunk's
 *   own slot of the scratch, by a fixed assignment of elements to lanes; one workgroup then sums the slots in a fixed order.  No float
 *   atomics: the result is bit-identical run to run and independent of grid size, stream and pointer alignment.  That workgroup writes
 *   the step record (gvf_optim_record, device): grad_norm = (float)sqrt(sum); found_inf = the sum is not finite;
 *   clip_coef = min(1, max_grad_norm / (grad_norm + 1e-6)) in fp32 as torch's clip_grad_norm_ rounds it (the reciprocal, then the
 *   product), 1 when max_grad_norm < 0;
 *   step += 1 only when the sum is finite; bc1 = 1 - beta1^step and 1 / sqrt(1 - beta2^step) in double; per group lr / bc1 in double,
 *   rounded to fp32 once.  The record's `step` is the optimizer's only state besides m and v; the caller zeroes the record once.
 *
 * gvf_optim_adamw_update (one launch) reads the record; per element, every operation rounded once to fp32 in this order
 * (gc = (g * inv_scale) * clip_coef; the coefficients 1-beta1, 1-beta2, 1-lr*wd, 1-rate are formed in double and rounded once):
 *     p = p * (1 - lr*wd)
 *     m = beta1 * m + (1-beta1) * gc
 *     v = beta2 * v + ((1-beta2) * gc) * gc
 *     p = p - ((lr/bc1) * m) / (sqrt(v) * (1/sqrt(bc2)) + eps)
 *     e_k = r_k * e_k + (1-r_k) * p                     for every EMA k
 * With found_inf set, p, m, v (and step) stay bit-for-bit unchanged and the EMAs still move toward the unchanged p (the reference's
 * update_ema runs after a skipped step as well).  Gradients are not zeroed here: that is one memset of the caller's flat buffer.
 * A tensor whose p, g, m, v and EMA bases are all 16-byte aligned moves in 16-byte accesses, any other one element by element.
 *
 * Conventions as in gvf_loss.h: device pointers, an explicit stream (null = the default stream), an int status, caller-owned buffers,
 * arguments checked on the host before any launch, nothing read back to the host.
 */
#ifndef GVF_OPTIM_H
#define GVF_OPTIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GVF_OPTIM_MAX_GROUPS 8
#define GVF_OPTIM_MAX_EMA 4

typedef struct gvf_optim_tensor {
    float* p;
    const float* g;
    float* m;
    float* v;
    float* ema[GVF_OPTIM_MAX_EMA];
    int32_t group;      /* 0 .. n_groups-1 */
    int32_t reserved;
} gvf_optim_tensor;     /* 72 bytes */

typedef struct gvf_optim_chunk {
    int32_t tensor;
    int32_t count;
    int64_t first;
} gvf_optim_chunk;      /* 16 bytes */

/* Host memory; read at the call.  Every value is a double: the derived coefficients are formed in double and rounded to fp32 once. */
typedef struct gvf_optim_hyper {
    int32_t n_groups;   /* 1 .. 8 */
    int32_t n_ema;      /* 0 .. 4 */
    double lr[GVF_OPTIM_MAX_GROUPS];
    double weight_decay[GVF_OPTIM_MAX_GROUPS];
    double beta1, beta2, eps;
    double ema_rate[GVF_OPTIM_MAX_EMA];
    double max_grad_norm;   /* < 0: no clipping */
} gvf_optim_hyper;

/* Device memory, 128 bytes, zeroed once by the caller; written by gvf_optim_norm, read by gvf_optim_adamw_update. */
typedef struct gvf_optim_record {
    float grad_norm;        /*  0 */
    int32_t found_inf;      /*  4 */
    float clip_coef;        /*  8 */
    float rsqrt_bc2;        /* 12: (float)(1 / sqrt(1 - beta2^step)) */
    int64_t step;           /* 16 */
    double bc1;             /* 24: 1 - beta1^step */
    double rsqrt_bc2_f64;   /* 32 */
    float step_size[GVF_OPTIM_MAX_GROUPS];   /* 40: (float)(lr / bc1) */
    char reserved[56];
} gvf_optim_record;

/* Elements per chunk (a multiple of 4). */
int gvf_optim_chunk_len(void);

/* Scratch of gvf_optim_norm for n_chunks chunks (one double per chunk).  GVF_EINVAL for n_chunks <= 0 or a null out. */
int gvf_optim_scratch_bytes(int64_t n_chunks, size_t* out);

/* GVF_EINVAL: a null table, hyper, record or scratch; n_tensors or n_chunks <= 0; n_groups outside 1..8; n_ema outside 0..4; a beta
 * outside [0, 1); eps <= 0; an EMA rate outside [0, 1]; a non-finite lr or weight decay; a nan max_grad_norm; scratch_bytes below
 * gvf_optim_scratch_bytes(n_chunks). */
int gvf_optim_norm(const gvf_optim_tensor* tensors, int n_tensors, const gvf_optim_chunk* chunks, int64_t n_chunks,
                   const gvf_optim_hyper* hyper, const float* inv_scale, gvf_optim_record* record, void* scratch, size_t scratch_bytes,
                   void* stream);

/* After gvf_optim_norm on the same stream with the same tables, hyper and inv_scale.  GVF_EINVAL as above (no scratch). */
int gvf_optim_adamw_update(const gvf_optim_tensor* tensors, int n_tensors, const gvf_optim_chunk* chunks, int64_t n_chunks,
                           const gvf_optim_hyper* hyper, const float* inv_scale, const gvf_optim_record* record, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GVF_OPTIM_H */
