/* libu2mkd_hip C ABI, continued: the fused SphereFormer / sptr window attention on 16-bit rows.
 *
 * Included by u2mkd_hip.h (inside its extern "C" block, behind the fp32 entries u2mkd_sptr_attention_forward_strided /
 * _backward_strided whose arguments these take); include that header, not this one.  The four entries live in a file of
 * their own because they are a row-type family of ONE operator: the Python side binds them from their own table
 * (u2mkd_amd/_lib.py: SPTR_ROWS16_SIGNATURES), and tests/test_sptr_rows16_cabi.py holds header, library and table together. */
#ifndef U2MKD_HIP_SPTR_ROWS16_H
#define U2MKD_HIP_SPTR_ROWS16_H
#ifndef U2MKD_HIP_H
#error "include u2mkd_hip.h, which includes this file"
#endif

/* The two strided entries on 16-BIT ROWS (bf16 / fp16 storage, see u2mkd_conv_forward_tiles_bf16 / _f16): q, k, v, out, dout, dq,
 * dk, dv point to bf16 / fp16 rows, ld_qkv, ld_out and ld_grad count ELEMENTS; every other argument as above.  The arithmetic is
 * the fp32 entries' (the reference upcasts before every sptr call, spherical_transformer.py:221-223): a 16-bit value is widened
 * exactly on load and a result rounded to nearest-even once at its store, so out equals the fp32 entry's out on the upcast rows
 * rounded once, and lse -- fp32, like delta, the tables, their gradients and the workspace -- equals it bit for bit.  An fp16
 * result beyond +-65504 is stored as +-inf, never saturated.  Rows move as 16-byte accesses: a stride that is no multiple of 8
 * elements or a row pointer that is not 16-byte aligned is an error (nothing is launched).  u2mkd_sptr_backward_workspace_bytes
 * and u2mkd_sptr_table_reduce are shared with the fp32 entries.                                                            */
int u2mkd_sptr_attention_forward_strided_bf16(const void *q, const void *k, const void *v, int64_t ld_qkv, float q_scale,
                                              const int32_t *sort_idx, const int32_t *wstart, const int32_t *wlen,
                                              const int32_t *qc, const float *radial, const float *tq, const float *tk,
                                              const float *tv, int32_t L, int32_t qgl, float split_a, int64_t n, int32_t h,
                                              int32_t hdim, void *out, int64_t ld_out, float *lse, u2mkd_stream_t s);
int u2mkd_sptr_attention_forward_strided_f16(const void *q, const void *k, const void *v, int64_t ld_qkv, float q_scale,
                                             const int32_t *sort_idx, const int32_t *wstart, const int32_t *wlen,
                                             const int32_t *qc, const float *radial, const float *tq, const float *tk,
                                             const float *tv, int32_t L, int32_t qgl, float split_a, int64_t n, int32_t h,
                                             int32_t hdim, void *out, int64_t ld_out, float *lse, u2mkd_stream_t s);
int u2mkd_sptr_attention_backward_strided_bf16(const void *q, const void *k, const void *v, int64_t ld_qkv, float q_scale,
                                               const void *out, const void *dout, int64_t ld_out, const float *lse,
                                               const int32_t *sort_idx, const int32_t *wstart, const int32_t *wlen,
                                               const int32_t *qc, const float *radial, const float *tq, const float *tk,
                                               const float *tv, int32_t L, int32_t qgl, float split_a, int32_t qc_span,
                                               int64_t n, int32_t h, int32_t hdim, float *delta /*[n,h] scratch*/,
                                               void *workspace, size_t workspace_bytes, void *dq, void *dk, void *dv,
                                               int64_t ld_grad, float *dtq, float *dtk, float *dtv, u2mkd_stream_t s);
int u2mkd_sptr_attention_backward_strided_f16(const void *q, const void *k, const void *v, int64_t ld_qkv, float q_scale,
                                              const void *out, const void *dout, int64_t ld_out, const float *lse,
                                              const int32_t *sort_idx, const int32_t *wstart, const int32_t *wlen,
                                              const int32_t *qc, const float *radial, const float *tq, const float *tk,
                                              const float *tv, int32_t L, int32_t qgl, float split_a, int32_t qc_span,
                                              int64_t n, int32_t h, int32_t hdim, float *delta /*[n,h] scratch*/,
                                              void *workspace, size_t workspace_bytes, void *dq, void *dk, void *dv,
                                              int64_t ld_grad, float *dtq, float *dtk, float *dtv, u2mkd_stream_t s);

#endif /* U2MKD_HIP_SPTR_ROWS16_H */
