/*
 * gvf_attn_bwd.h -- C ABI of the attention backward (csrc/attn_bwd.hip): dQ, dK, dV of
 *     out = softmax(q k^T * scale) v,     head_dim 32 or 64, no mask, no dropout, scale > 0,
 * the gradient of gvf_attn_fwd (gvf_dit.h) without its fused RMSNorm gains and with row-major v.
 *
 * Tensors are 16-bit (`dtype`: GVF_DT_BF16 / GVF_DT_F16 of gvf_dit.h) and addressed as in gvf_attn_fwd: batch index = (outer, inner),
 * 4 strides in elements {outer, inner, seq, head}, element (o,i,l,h,c) at o*s[0] + i*s[1] + l*s[2] + h*s[3] + c, so the q / k / v
 * slices of a packed qkv or kv projection are read in place.  q, out, dout, dq have Lq rows, k, v, dk, dv have Lk rows; any
 * lengths >= 1.  Input bases and strides keep 16-byte alignment (8 elements), gradient bases and strides 8 bytes (4 elements).
 *
 * Method: P is recomputed from q, k and a per-row log-sum-exp.  A statistics pass writes lse2 = log2 sum_k exp2(c s_k), c = scale log2 e,
 * and delta = sum_d dout_d out_d (fp32, (N, H, Lq) each) into the workspace; one sweep has a workgroup own a key block and walk the
 * queries (dk, dv), one has it own a query block and walk the keys (dq).  Sequences with Lq, Lk <= 32 and head_dim 32 take one wave
 * per (sequence, head) and touch no workspace.
 * Rounding: scores and dP = dout v^T fp32 from the 16-bit operands; p = exp2(c s - lse2) fp32, rounded to 16 bit where it feeds dv;
 * dS = p (dP - delta) scale rounded to 16 bit where it feeds dq and dk; fp32 accumulation; gradients stored in the operand type.
 * With few key blocks and many queries the key sweep splits the query range over several workgroups per key block, by a rule of the
 * shape alone; their fp32 partial dk / dv (in the workspace) are added in chunk order by one more kernel and rounded once.
 * Determinism: every gradient element is summed in a fixed order -- no float atomics, no waiting between workgroups -- so two calls
 * on the same inputs give bit-identical gradients.
 *
 * Conventions as in gvf_loss.h: device pointers, an explicit stream (null = the default stream), no host synchronisation and no
 * allocation, an int status.  Every argument is checked on the host before any launch; GVF_EINVAL for a null pointer, a head_dim
 * other than 32 / 64, a dtype that is not a 16-bit type, a non-positive count or length, a misaligned base or stride, scale <= 0,
 * or a workspace smaller than gvf_attn_bwd_workspace_bytes reports.
 */
#ifndef GVF_ATTN_BWD_H
#define GVF_ATTN_BWD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the caller-owned workspace of one gvf_attn_bwd call (the row statistics and, for a split key sweep, the partial
 * sums): host only.  The workspace must be 16-byte aligned. */
int gvf_attn_bwd_workspace_bytes(int n_outer, int n_inner, int Lq, int Lk, int H, int head_dim, size_t* out);

int gvf_attn_bwd(int dtype, const void* q, const void* k, const void* v, const void* out, const void* dout,
                 void* dq, void* dk, void* dv,
                 int n_outer, int n_inner, int Lq, int Lk, int H, int head_dim,
                 const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides, const int64_t* o_strides,
                 const int64_t* do_strides, const int64_t* dq_strides, const int64_t* dk_strides, const int64_t* dv_strides,
                 float scale, void* workspace, size_t workspace_bytes, void* stream);

/*
 * The ragged form: the gradient of gvf_attn_varlen_fwd (gvf_dit.h) without gains.  Tensors are packed [T, H, C] token lists addressed as
 * there: 4 strides {outer (normally 0), inner (unused), seq, head}, sequence s owns token rows [cu[s], cu[s + 1]) and its element
 * (l, h, c) sits at s * st[0] + (cu[s] + l) * st[2] + h * st[3] + c.  q, out, dout, dq have total_q rows and follow cu_seqlens_q;
 * k, v, dk, dv have total_k rows and follow cu_seqlens_k.  cu_seqlens_* are device int32 [n_seqs + 1], non-decreasing, starting at 0
 * and ending at the total; they are read on the device only -- no length crosses to the host, no allocation, no synchronisation.
 * max_Lq / max_Lk (>= 1) size the grids: a value below a real length is outside the contract (rows past it get no gradient), as in
 * the forward.  Alignment, scale, dtype and head_dim as for gvf_attn_bwd; the same host checks, plus GVF_EINVAL for a null cu_seqlens,
 * n_seqs, H or max_L* <= 0, and a total that is negative or above 2^31 - 1.
 *
 * Method, rounding points and determinism are gvf_attn_bwd's: the same kernels with another problem decode (the short-sequence kernel
 * is not used).  Workspace: lse2 and delta, fp32 [H][total_q] each (256-byte aligned), then, when the key sweep is split, its fp32
 * partials [2][split][H][total_k][head_dim].  The split count is a function of n_seqs, H, max_Lq, max_Lk and head_dim alone: the dense
 * rule applied to n_seqs * H problems of the longest lengths.  Every sequence's own query tiles are divided over the chunks in order; a
 * chunk that holds none of them contributes zeros, and the chunks are summed in chunk order.
 * Empty sequences: queries without keys get dq = +0 (the forward wrote zero output rows); keys without queries get dk = dv = +0.
 */
int gvf_attn_varlen_bwd_workspace_bytes(int n_seqs, long long total_q, long long total_k, int max_Lq, int max_Lk, int H, int head_dim,
                                        size_t* out);

int gvf_attn_varlen_bwd(int dtype, const void* q, const void* k, const void* v, const void* out, const void* dout,
                        void* dq, void* dk, void* dv,
                        int n_seqs, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k,
                        long long total_q, long long total_k, int max_Lq, int max_Lk, int H, int head_dim,
                        const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides, const int64_t* o_strides,
                        const int64_t* do_strides, const int64_t* dq_strides, const int64_t* dk_strides, const int64_t* dv_strides,
                        float scale, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GVF_ATTN_BWD_H */
