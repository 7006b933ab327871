/*
 * gsdd.h — C ABI of the MI355X (gfx950) video-token generation hot path.
 *
 * Drop-in boundary for the VQ-VAE encode/quantise/decode + D3PM reverse-diffusion path of
 * Developer-Zer0/GIF-synthesis-with-Discrete-Diffusion.  The reference has NO native FFI for this
 * path: its seam is Hydra `_target_` instantiation of torch nn.Modules.  Each entry
 * point below therefore cites the reference *op sequence* (file:line under /root/reference) that
 * it replaces; the Python shells in gif-synthesis-with-discrete-diffusion_amd/ bind them with ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc'd / torch-ROCm storage); the library never
 *     allocates, frees or synchronises; all work is enqueued on `stream` (a hipStream_t passed as void*).
 *   - fp32 everywhere; token / code indices are int64 (torch.argmin/argmax dtype).
 *   - return 0 on success, <0 on error (GSDD_E_*); gsdd_last_error() gives a message (thread-local).
 *   - activations are channels-last: a "row" is one position (n,t,h,w) with C contiguous floats.
 *   - arithmetic mode / kernel variant are ARGUMENTS (a `mode` / `variant` / `flags` value, 0 = the documented default), chosen per
 *     call and therefore per stream; the library reads no environment variable and keeps no mode latched in static state.  (The
 *     Python shells map their GSDD_* debugging environment variables onto these arguments: gif-synthesis-with-discrete-diffusion_amd/ops.py.)
 */
#ifndef GSDD_H
#define GSDD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSDD_OK 0
#define GSDD_E_ARG (-1)     /* bad argument (null pointer, unsupported shape)  */
#define GSDD_E_HIP (-2)     /* a HIP runtime call failed                        */
#define GSDD_E_STATE (-3)   /* graph capture misuse                             */
#define GSDD_E_CAP (-4)     /* a host output buffer is too small                */

const char* gsdd_last_error(void);
int gsdd_version(void);
/* sizeof of a descriptor struct as this build of the library sees it (which: 0 gsdd_gemm_desc, 1 gsdd_layer_desc, 2 gsdd_step_desc,
 * 3 gsdd_train_desc, 4 gsdd_purity_desc, 5 gsdd_purity_select_desc, 7 gsdd_jump_desc, 8 gsdd_optim_state, 10 gsdd_compose_desc; anything else, 6 and 9 included: -1).  A binding checks its own struct sizes against these when it loads the library, so that a
 * library built from another revision of this header fails at load time instead of misreading a descriptor. */
int64_t gsdd_abi_sizeof(int which);

/* ------------------------------------------------------------------ generic implicit GEMM
 * out[orow(m)][n] = epi( sum_{tap,c} pro(in[src(m,tap)][c]) * w[tap][n][c] )
 * One kernel serves every dense contraction on the VQ-VAE path and the denoiser's linears:
 *   SamePadConv3d / nn.Conv3d            videogpt_vq_vae.py:289-309   (taps = kt*kh*kw)
 *   SamePadConvTranspose3d (per phase)   videogpt_vq_vae.py:312-332   (sub-pixel phases)
 *   nn.Linear                            model_utils.py:223-233, transformer_utils.py:36-43,258-263,353-356
 * Activation modes (act):  0 none, 1 ReLU, 2 x*sigmoid(1.702x) (GELU2, transformer_utils.py:115-119)
 */
typedef struct {
    /* input tensor: N x Di x Hi x Wi positions, row pitch `in_pitch` floats, Cin used channels */
    const float* in;
    int N, Di, Hi, Wi, Cin, in_pitch;
    /* output grid (positions enumerated (n,to,ho,wo)); rows M = N*Do*Ho*Wo */
    int Do, Ho, Wo;
    int sd, sh, sw;                 /* input stride per output step                          */
    int ntaps;
    const int* taps;                /* device int[ntaps*3]: (dt,dh,dw) added to o*stride     */
    const int64_t* gather;          /* optional: in row = gather[m] (ntaps must be 1)        */
    /* weights: [ntaps][Cout][Cin] floats (Cin contiguous) */
    const float* w;
    int Cout;
    /* prologue on the input operand */
    const float* pro_scale;         /* per input channel a = relu(x*ps[c]+pb[c]) (BN+ReLU)   */
    const float* pro_shift;
    const float* ln_stats;          /* per input row (mean, rstd) pairs -> LayerNorm         */
    const float* ln_gamma;          /* [sel][Cin]   a = (x-mu)*rs*gamma + beta               */
    const float* ln_beta;
    const int64_t* ln_sel;          /* optional per-batch selector (e.g. timestep), else 0   */
    int ln_stride;                  /* floats between selector rows                          */
    int rows_per_batch;             /* rows per batch element (for ln_sel / bvec)            */
    /* epilogue */
    const float* epi_scale;         /* per output channel, optional                          */
    const float* epi_shift;         /* per output channel (bias / folded BN), optional       */
    const float* bvec;              /* optional [batch][Cout] vector added per batch element */
    int act;
    const float* residual;          /* optional, same addressing as out                      */
    /* output addressing: row = ((n*oD + to*osd+ood)*oH + ho*osh+ooh)*oW + wo*osw+oow         */
    float* out;
    int oD, oH, oW, osd, osh, osw, ood, ooh, oow, out_pitch;
    int out_mode;                   /* 0 channels-last rows; 1 NCDHW (out[n][c][d][h][w]);
                                       2 head-major [n/4][M][4] (denoiser q/k/v)             */
    int flags;                      /* 0, or GSDD_GEMM_EXACT_F32                             */
} gsdd_gemm_desc;
/* flags: contractions of 64 or more run as error-free 3-way bf16 splits on the matrix pipe by default (six cross products, dropped
 * terms < 2^-24 relative); GSDD_GEMM_EXACT_F32 runs them on v_mfma_f32_32x32x2_f32 (an fmaf chain in f32) instead -- also honoured by
 * gsdd_conv_wgrad. */
#define GSDD_GEMM_EXACT_F32 1
int gsdd_gemm(const gsdd_gemm_desc* d, void* stream);

/* per-row LayerNorm statistics (mean, rstd) of x[M][C] (eps inside rsqrt).
 * Replaces the statistics half of nn.LayerNorm: transformer_utils.py:147,157,217,354 */
int gsdd_row_stats(const float* x, int64_t M, int C, float eps, float* stats, void* stream);
/* y[m][:] = (x[m][:] - mean) * rstd * gamma + beta with stats from gsdd_row_stats: LayerNorm rows of any width C % 4 == 0 as an
 * output of their own (the text tower's per-token features; elsewhere the normalisation is a GEMM prologue, and gsdd_ln_fwd, which
 * writes normalised rows too, takes C == 64 only while the tower is 512 wide). */
int gsdd_ln_apply(const float* x, const float* stats, const float* gamma, const float* beta, int64_t M, int C, float* y, void* stream);

/* ------------------------------------------------------------------ layout at the NCDHW boundary
 * videogpt_vq_vae.py:58-60 hands (B,3,T,H,W); kernels are channels-last. */
int gsdd_ncdhw_to_rows(const float* x, int N, int C, int D, int H, int W, int Cpad, int padw,
                       float* out, void* stream);

/* ------------------------------------------------------------------ VQ-VAE specific
 * Axial attention over one axis of a (N,T,H,W) grid of fused q|k|v rows.
 * qkv row layout: [9*C] = (axis a: q,k,v) for a in (w,h,t); out row layout [3*C] = (a_w|a_h|a_t).
 * Replaces AxialAttention + scaled_dot_product_attention: model_utils.py:318-337, :586-600. */
#define GSDD_AXIAL_AUTO 0           /* register-resident MFMA kernel where the line length and head dim allow (16-position lines) */
#define GSDD_AXIAL_VALU 1           /* the LDS / vector kernel for every axis: the cross-check variant                            */
int gsdd_axial_attention(const float* qkv, int N, int T, int H, int W, int C, int n_head,
                         float* out, int variant, void* stream);
/* Shapes.  gsdd_axial_attention and gsdd_axial_attention_bwd accept exactly the same (T, H, W, C, n_head), whatever the variant:
 * C % n_head == 0 and, with d = C / n_head, every axis length S in 1 .. 64 with (4 S (d + 1) + 2 S^2) * 4 <= 163,840 -- the bytes
 * of LDS the backward LDS kernel keeps per (line, head) against the 160 KiB of a workgroup (the forward keeps (3 S (d + 1) + S^2) * 4,
 * never more).  That is every S <= 64 at d <= 64, S <= 63 at d = 128, S <= 37 at d = 256.  Anything else is GSDD_E_ARG from both,
 * decided for all three axes before the first launch: a refused call has written nothing.
 * gsdd_axial_attention_lds_bytes: those bytes (backward != 0: of the backward kernel) for one axis, or -1 where (S, d) is refused. */
int64_t gsdd_axial_attention_lds_bytes(int S, int d, int backward);

/* Nearest codebook entry: idx[m] = argmin_k (|z_m|^2 - 2 z_m.e_k + |e_k|^2), first minimum wins.
 * Replaces Codebook.forward distance+argmin: videogpt_vq_vae.py:178-183.
 * z: [M][E] rows, cb: [K][E]; optional zq[M][E] = cb[idx] (the F.embedding at :186).
 * workspace: gsdd_nearest_code_workspace_bytes(K) bytes (the |e_k|^2 vector).  With it, E == 128 and K % 32 == 0 the distances
 * are a GEMM on the f32 matrix cores with the arg-min as its epilogue (never materialised); otherwise, or with workspace ==
 * NULL, the register-tiled vector kernel runs (any E % 4 == 0, any K). */
int64_t gsdd_nearest_code_workspace_bytes(int K);
int gsdd_nearest_code(const float* z, int64_t M, int E, const float* cb, int K,
                      int64_t* idx, float* zq, void* workspace, int64_t workspace_bytes, void* stream);

/* 3-D max / mean pooling on channels-last rows, for the FVD evaluator's I3D feature extractor (MaxPool3dSamePadding and the
 * final AvgPool3d: src/models/motionencoder/pytorch_i3d.py:7-34, :296).  in: N x Di x Hi x Wi positions of `in_pitch` floats, C of
 * them pooled; window kernel[3] / stride[3] starting at o * stride - pad_front; out grid Do x Ho x Wo with row pitch out_pitch
 * (a channel slice of a wider concatenated row is addressed by offsetting `out`).  mode 0: maximum, positions outside the input
 * count as 0 (the reference zero-pads, then pools unpadded); mode 1: mean over the full window. */
int gsdd_pool3d(const float* in, int N, int Di, int Hi, int Wi, int C, int in_pitch, const int* kernel, const int* stride,
                const int* pad_front, int Do, int Ho, int Wo, int mode, float* out, int out_pitch, void* stream);

/* ------------------------------------------------------------------ VQ-VAE train-mode forward pieces
 * nn.BatchNorm3d in train mode on rows x[M][C] (videogpt_vq_vae.py:125-133, 242-247): batch mean / biased variance ->
 * folded scale = w/sqrt(var+eps), shift = b - mean*scale (consumed by gsdd_gemm's pro_scale/pro_shift); running stats
 * (may be NULL) updated with momentum and the unbiased variance like torch. */
int64_t gsdd_bn_train_workspace_bytes(int64_t M, int C);
int gsdd_bn_train(const float* x, int64_t M, int C, const float* weight, const float* bias, float eps, float momentum,
                  float* running_mean, float* running_var, float* scale, float* shift, float* mean_rstd /* optional [C][2] */,
                  void* workspace, int64_t workspace_bytes, void* stream);

/* Codebook EMA (Codebook.forward, videogpt_vq_vae.py:193-214) in two phases so the caller can all-reduce between them
 * (:196-198): phase 0: n_total[K], encode_sum[K][E] from (z rows, idx); phase 1: N, z_avg EMA with `decay`, Laplace-
 * smoothed embeddings, dead codes (N < 1) restarted from z[perm[k]] (:205-214).  scalars[0] = sum(N), scalars[1] =
 * exp(-H(n_total / M)) (the perplexity when n_total is this rank's own count over M latents; otherwise use
 * gsdd_code_perplexity on the local counts). */
int gsdd_codebook_ema(const float* z, const int64_t* idx, int64_t M, int E, int K, float decay, const int64_t* perm,
                      float* N, float* z_avg, float* embeddings, float* n_total, float* encode_sum, float* scalars,
                      int phase, void* stream);

/* out[0] = exp(-sum_k p_k log(p_k + 1e-10)), p_k = n_local[k] / M: the codebook perplexity of THIS rank's M latents
 * (videogpt_vq_vae.py:218-219 take the mean of the local one-hot, before any all-reduce and before _tile). */
int gsdd_code_perplexity(const float* n_local, int K, int64_t M, float* out, void* stream);

/* out[0] = scale * mean((a-b)^2), deterministic fp64 two-stage reduction (F.mse_loss at videogpt_vq_vae.py:64, :190);
 * workspace >= 8 KiB. */
int gsdd_mse(const float* a, const float* b, int64_t n, float scale, float* out, void* workspace, int64_t workspace_bytes,
             void* stream);

/* ------------------------------------------------------------------ VQ-VAE training step: backward building blocks
 * (autograd of videogpt_vq_vae.py:102-138, 228-332; data gradients of (transposed) convolutions are gsdd_gemm calls with
 * transposed weights and mirrored tap tables) */
/* dW[tap][n][c] += sum_m dY[orow(m)][n] * pro(in[src(m,tap)][c]); geometry / taps / BN+ReLU prologue / dY row addressing
 * (the output-addressing fields) taken from the forward descriptor; Cout and dy_pitch multiples of 4. */
int gsdd_conv_wgrad(const gsdd_gemm_desc* d, const float* dY, int dy_pitch, float* dW, void* stream);
/* a = relu(BatchNorm_train(x)) backward: given da -> dx (= dx_in + ...), dgamma += , dbeta += */
int64_t gsdd_bn_relu_bwd_workspace_bytes(int64_t M, int C);
int gsdd_bn_relu_bwd(const float* da, const float* x, int64_t M, int C, const float* mean_rstd, const float* gamma,
                     const float* beta, const float* dx_in, float* dx, float* dgamma, float* dbeta, void* workspace,
                     int64_t workspace_bytes, void* stream);
/* dpre = dout * [out > 0] */
int gsdd_relu_mask(const float* dout, const float* out, float* dpre, int64_t n, void* stream);
/* out = (a ? a : 0) + alpha * (b - c) */
int gsdd_lincomb(const float* a, const float* b, const float* c, float alpha, float* out, int64_t n, void* stream);
/* backward of gsdd_axial_attention: datt rows [M][3C] -> dqkv rows [M][9C] */
int gsdd_axial_attention_bwd(const float* qkv, const float* datt, int N, int T, int H, int W, int C, int n_head, float* dqkv,
                             int variant /* GSDD_AXIAL_* */, void* stream);

/* ------------------------------------------------------------------ D3PM denoiser pieces
 * x[b][l][:] = emb[tok[b][l]] + pos[l]   (DalleMaskImageEmbedding.forward, dalle_mask_image_embedding.py:59-79;
 * pos = height_emb[l/W]+width_emb[l%W] precomputed once). rep: x is written for `rep` stacked copies. */
int gsdd_d3pm_embed(const int64_t* tok, int B, int L, int D, const float* emb, int n_embed,
                    const float* pos, int rep, float* x, void* stream);

/* AdaLayerNorm modulation table: out[t][0:D] = 1+scale, out[t][D:2D] = shift with
 * [scale|shift] = Linear(SiLU(emb[t]))  (AdaLayerNorm, transformer_utils.py:138-159). */
int gsdd_adaln_table(const float* emb, int T, int D, const float* lin_w, const float* lin_b,
                     float* out, void* stream);

/* y[r][:] = W x[r] + b for a handful of rows (cross-attention value/proj of the condition token,
 * transformer_utils.py:95-113 with T_E == 1: softmax over one key == 1). */
int gsdd_small_linear(const float* x, int R, int Cin, const float* w, const float* b, int Cout,
                      float* y, void* stream);

/* Self-attention for head dim 4: q,k,v head-major [H][M][4] (M = B*L rows), out rows [M][H*4].
 * softmax(q k^T / sqrt(4)) v, scores never leave registers.
 * Replaces FullAttention.forward: transformer_utils.py:46-62 (head-mean att is dropped: unused). */
/* workspace: gsdd_d3pm_attention_workspace_bytes(B,L,H) bytes of scratch for the matrix-pipe kernel: the pre-split K image
 * (32 B per key and head), the V image (32 B) and, per (head, 32-key pair-tile), the sum of the tile's keys (float4) and one f32
 * bounding the tile's largest ||k||.  The norms let the kernel prove from ||q|| ||k|| alone that a tile holds no probability above
 * 2^-8 of its row sum (then only the f16 hi half of P is used for it); the sums give it the mean key, hence a lower bound of every
 * final row sum before a key has been seen.  Behind them, 32-byte aligned, 32 B per (batch row, head): the
 * sum of all its keys (float4), its largest tile norm, an inf / NaN flag and two zero words -- what the adaptive kernels need of a
 * whole (b, h), reduced from the per-tile numbers by one small launch ahead of them (they read nothing else of the kind; the other
 * modes never touch these bytes).  Layout: K image | V image | key sums | tile norms | (b, h) records.  NULL selects the
 * workspace-free kernel (exact-f32 P.V on v_mfma_f32_4x4x1). */
int64_t gsdd_d3pm_attention_workspace_bytes(int B, int L, int H);
/* k = v = NULL: the workspace already holds the images, key sums and norms (written by gsdd_d3pm_layer through kv_img).
 * redo_events: optional device counter (caller-owned, caller-zeroed) to which the kernel adds one per (wave, chunk) it had to
 * redo with a larger exponent offset after an f16 overflow -- the kernel's only other data-dependent cost, 0 for near-uniform
 * attention rows.  The library keeps no counter of its own (no hidden global state). */
/* mode: how the softmax probabilities P enter the P.V product on the f16 matrix pipe (errors and times: DESIGN.md section 4).
 *   GSDD_ATTN_AUTO   GSDD_ATTN_A8 for L >= 2048, GSDD_ATTN_P22 below (short rows have too few keys to average the skipped halves out)
 *   GSDD_ATTN_P22    f16 hi + lo (22 bits) in every tile: the most exact variant (output within 2e-6 of fp64)
 *   GSDD_ATTN_P11    f16 hi only (11 bits) in every tile: the fastest; relative error of a probability <= 2^-12, output error up to
 *                    ~1.4e-4 |v - o| / sqrt(effective keys per row) -- within the path's 1e-4 logits contract on every pinned case
 *                    (tests/test_gpu_parity.py, tests/test_gpu_fullsize.py), but not within this kernel's own 2e-5 bar on peaked rows
 *   GSDD_ATTN_A8     adaptive: lo half only in (16-query, 32-key) tiles that can hold a probability above 2^-8 of the row sum
 *   GSDD_ATTN_A12    the same with threshold 2^-12
 *   GSDD_ATTN_F32PV  the workspace-free kernel (exact-f32 P.V) even when a workspace is given (k, v must be given)
 *   GSDD_ATTN_KC256  development variant: 256-key chunks, hi + lo everywhere
 * GSDD_ATTN_NOLEAN may be OR-ed into any of them (here and in gsdd_d3pm_attention_train): the adaptive kernels then send every wave
 * through the general chunk loop, also the "quiet" waves whose bounds prove up front that no tile needs a lo half and no f16 can
 * overflow and which otherwise take a loop without that bookkeeping.  Same bits either way: for tests and A/B timing. */
#define GSDD_ATTN_AUTO 0
#define GSDD_ATTN_P22 1
#define GSDD_ATTN_P11 2
#define GSDD_ATTN_A8 3
#define GSDD_ATTN_A12 4
#define GSDD_ATTN_F32PV 5
#define GSDD_ATTN_KC256 6
#define GSDD_ATTN_NOLEAN 256
int gsdd_d3pm_attention(const float* q, const float* k, const float* v, int B, int L, int H,
                        float* out, void* workspace, int64_t workspace_bytes, uint64_t* redo_events, int mode, void* stream);

/* Fused post-attention half of a denoiser block (n_embd 64, hidden 256), rows updated in place:
 *   x += proj(y)+b_proj+cvec[b];  x += W2 GELU2(W1 LN2(x)+b1)+b2;  [qkv_next = Wqkv AdaLN_next(x,t)+b_qkv, head-major]
 * Replaces Block.forward's tail (transformer_utils.py:268-282: attn1 proj + residual, T_E==1 cross-attention
 * vector, ln2, mlp :258-263, residual) and the next block's AdaLayerNorm (:150-159) + query/key/value (:48-50).
 * qkv == NULL skips the next-block stage (last block). */
typedef struct {
    const float* y;             /* [M][64] attention output                         */
    float* x;                   /* [M][64] residual stream, in/out                  */
    int64_t M;
    int L;                      /* rows per batch element                           */
    int n_embd, hidden;         /* must be 64, 256                                  */
    const float* cvec;          /* optional [M/L][64] per-batch vector              */
    const float* wproj; const float* bproj;
    const float* ln2_g; const float* ln2_b;
    const float* w1; const float* b1;     /* [256][64], [256]                       */
    const float* w2; const float* b2;     /* [64][256], [64]                        */
    const float* ada;           /* next block: [T][128] (1+scale | shift) table     */
    const int64_t* t2;          /* device int64[M/L] timesteps                      */
    const float* wqkv; const float* bqkv; /* [192][64], [192]                       */
    float* qkv;                 /* [48][M][4] or NULL                               */
    const void* w2_x3;          /* gsdd_d3pm_layer_pack images (bf16x3 MFMA fragments) of this block's w2 + wproj and of the */
    const void* wqkv_x3;        /* next block's wqkv: ready-made matrix operands streamed through LDS.  One of the two image */
                                /* sets (these or layer_h2 / wqkv_h2) must be given                                           */
    int64_t kv_img_bytes;       /* size of kv_img in bytes: at least gsdd_d3pm_attention_workspace_bytes(M / L, L, 16)          */
    void* kv_img;               /* optional (L % 32 == 0): the attention workspace of the next                                  */
                                /* block.  k and v are then written there as the matrix-pipe kernel's pre-split images instead */
                                /* of f32 rows of qkv, and gsdd_d3pm_attention is called with k = v = NULL (no prep pass)      */
    const void* layer_h2;       /* optional: gsdd_d3pm_layer_pack_h2 images (f16 hi + lo MFMA fragments) of this block's w1, w2 and */
    const void* wqkv_h2;        /* wproj, and of the next block's wqkv.  Preferred over the bf16x3 images when given: all three    */
                                /* weight matrices of the block are then LDS-resident and every product is 3 matrix instructions   */
                                /* instead of 6; as accurate as an f32 GEMM with f32 accumulation (22-bit operands, exact products) */
    int variant;                /* GSDD_LAYER_AUTO (the f16 hi + lo kernel when its images are given, else the bf16x3 one), or one of */
                                /* them explicitly: GSDD_LAYER_H2 / GSDD_LAYER_X3P (an error if that kernel's images are missing)    */
    int* range_flag;            /* optional device int (caller-zeroed), used by the f16 hi + lo kernel only: its operands are 16 a as  */
                                /* f16, so an activation |a| >= 4094 overflows to inf.  The kernel sets *range_flag = 1 when a row of  */
                                /* x it writes is not finite (inf / NaN propagate there); the caller then reruns with the bf16x3       */
                                /* images, which have f32's range (d3pm.py does: checked once per sample(), outside graph capture)    */
} gsdd_layer_desc;
#define GSDD_LAYER_AUTO 0
#define GSDD_LAYER_X3P 2
#define GSDD_LAYER_H2 3
int gsdd_d3pm_layer(const gsdd_layer_desc* d, void* stream);
/* Pre-split w2 [64][256] + wproj [64][64] (-> layer_x3, GSDD_LAYER_X3_BYTES) and wqkv [192][64] (-> wqkv_x3,
 * GSDD_LAYER_WQKV_X3_BYTES; both may be NULL) into the fragment images gsdd_d3pm_layer consumes; valid until the weights change. */
#define GSDD_LAYER_X3_BYTES (40 * 3 * 1024)
#define GSDD_LAYER_WQKV_X3_BYTES (24 * 3 * 1024)
int gsdd_d3pm_layer_pack(const float* w2, const float* wproj, const float* wqkv, void* layer_x3, void* wqkv_x3, void* stream);
/* The f16 hi + lo images: w1 [256][64] + w2 [64][256] + wproj [64][64] -> layer_h2 (GSDD_LAYER_H2_BYTES), wqkv [192][64] -> wqkv_h2
 * (GSDD_LAYER_WQKV_H2_BYTES); either image may be NULL (then its sources may be too).  Weights must be below 255 in magnitude. */
#define GSDD_LAYER_H2_BYTES (72 * 2 * 1024)
#define GSDD_LAYER_WQKV_H2_BYTES (24 * 2 * 1024)
int gsdd_d3pm_layer_pack_h2(const float* w1, const float* w2, const float* wproj, const float* wqkv, void* layer_h2, void* wqkv_h2,
                            void* stream);

/* Row GEMMs of a block in the training step: out[m][:] = x[m] W'^T + bias [+ bvec[m / rows_per_batch]] [+ residual[m]], n_in -> n_out
 * one of 64 -> 64 / 128 / 192 / 256 or 128 / 192 / 256 -> 64, with W' (n_out x n_in) given as a bf16x3 fragment image of
 * GSDD_ROWS_LINEAR_IMAGE_BYTES(n_out, n_in) bytes.  Replaces the nn.Linear calls of Block / FullAttention (transformer_utils.py:48-50,
 * 60, 258-263) and their data gradients in D3PMTrainer; head_major: out is [n_out / 4][M][4] (q | k | v).
 * gsdd_rows_linear_pack_many fills n_desc images in one launch from a DEVICE array of
 *   struct { const float* w; int n_out, n_in, ld, transpose; void* image; }   (transpose: W'[n][k] = w[k * ld + n], the data gradient's
 * operand; else W'[n][k] = w[n * ld + k]); max_out / max_in: the largest n_out / n_in among them. */
#define GSDD_ROWS_LINEAR_IMAGE_BYTES(n_out, n_in) ((n_out) / 64 * ((n_in) / 64) * 8 * 3 * 1024)
int gsdd_rows_linear_pack_many(const void* descs_dev, int n_desc, int max_out, int max_in, void* stream);
int gsdd_rows_linear(const float* x, int64_t M, int n_in, const void* image, int n_out, const float* bias, const float* bvec,
                     int rows_per_batch, const float* residual, float* out, int head_major, void* stream);

/* to_logits: out[m][:] = W LayerNorm(x[m]) + bias  (nn.LayerNorm + nn.Linear, transformer_utils.py:353-356, 442);
 * x: [M][64], w: [K][64], out: [M][K] rows (the reference's (B,K,L) is a transposed view of this). */
int gsdd_d3pm_logits(const float* x, int64_t M, int n_embd, const float* ln_g, const float* ln_b, const float* w,
                     const float* bias, int K, float* out, void* stream);

/* General cross-attention (T_E condition tokens), head dim 4; q head-major [H][M][4],
 * kc/vc rows [B*Te][H*4]; out rows [M][H*4].  transformer_utils.py:95-113. */
int gsdd_d3pm_cross_attention(const float* q, const float* kc, const float* vc, int B, int L, int Te,
                              int H, float* out, void* stream);

/* The same cross-attention for training (1 <= Te <= 77, anything else is GSDD_E_ARG).  The forward also writes lse[H][M], the
 * log-sum-exp per (head, row) in the log2 domain (as gsdd_d3pm_attention_train keeps it).  The backward takes the forward's out as o
 * and OVERWRITES dq (head-major [H][M][4]), dkc and dvc (rows [B*Te][H*4]); exact f32.  dkc / dvc are sums over the L rows of a batch
 * element: per-chunk partials go into the caller's workspace (gsdd_d3pm_cross_attention_bwd_workspace_bytes) and are added in a fixed
 * order -- no atomics, the same bits on every run, and a batch element's results do not depend on the others in the launch. */
int gsdd_d3pm_cross_attention_train(const float* q, const float* kc, const float* vc, int B, int L, int Te, int H, float* out,
                                    float* lse, void* stream);
int64_t gsdd_d3pm_cross_attention_bwd_workspace_bytes(int B, int L, int Te, int H);
int gsdd_d3pm_cross_attention_bwd(const float* q, const float* kc, const float* vc, const float* o, const float* dO,
                                  const float* lse, int B, int L, int Te, int H, float* dq, float* dkc, float* dvc,
                                  void* workspace, int64_t workspace_bytes, void* stream);

/* The three cross-attentions with a condition length per batch element (caption padding): batch element b attends to its keys
 * 0 .. cond_len[b] - 1 only.  The softmax runs over those keys; kc / vc rows at e >= cond_len[b] are NOT READ (they may hold anything,
 * NaN included), and the backward writes the dkc / dvc rows at e >= cond_len[b] as exact zeros (it still overwrites every row: no
 * atomics, fixed summation order, a batch element's results independent of the others in the launch).  The kernels are the ones of
 * the entry points above, which are their "every length is Te" case: cond_len[b] == Te for every b gives the same bits.
 * `cond_len` is a device int32 [B].  `cond_len_host` is, like eot_host of gsdd_text_pool, an optional HOST copy of the same integers:
 * when given, every entry is checked before the launch and a value outside [1, Te] is GSDD_E_ARG (gsdd_last_error names the index and
 * the value); when NULL (a captured step has no host copy) the kernels clamp the device value into [1, Te], so they never read outside
 * the rows and never divide by an empty sum.  1 <= Te <= 77; the workspace is the one gsdd_d3pm_cross_attention_bwd_workspace_bytes
 * sizes.  Training: the weight gradients of the key / value projections multiply the zero dkc / dvc rows by the condition rows, so the
 * condition rows behind a length must be FINITE there (0 x NaN is not 0). */
int gsdd_d3pm_cross_attention_len(const float* q, const float* kc, const float* vc, const int32_t* cond_len,
                                  const int32_t* cond_len_host, int B, int L, int Te, int H, float* out, void* stream);
int gsdd_d3pm_cross_attention_train_len(const float* q, const float* kc, const float* vc, const int32_t* cond_len,
                                        const int32_t* cond_len_host, int B, int L, int Te, int H, float* out, float* lse,
                                        void* stream);
int gsdd_d3pm_cross_attention_bwd_len(const float* q, const float* kc, const float* vc, const float* o, const float* dO,
                                      const float* lse, const int32_t* cond_len, const int32_t* cond_len_host, int B, int L, int Te,
                                      int H, float* dq, float* dkc, float* dvc, void* workspace, int64_t workspace_bytes, void* stream);

/* One fused reverse-diffusion step on int64 tokens:
 *   predict_start (fp log_softmax, clamp) x2 -> cf guidance mix -> q_posterior -> Gumbel arg-max.
 * Replaces diffusion_transformer.py:220-249 (predict_start/cf_predict_start tails), :251-283
 * (q_posterior), :354-359 (log_sample_categorical) and the log-one-hot round trip (:44-54).
 * logits_c / logits_u: [B*L][K] rows (logits_u may be NULL -> no guidance: predict_start only).
 * sched: 8 device arrays in the order log_at, log_bt, log_ct, log_1_min_ct (T each),
 *        log_cumprod_at, log_cumprod_bt, log_cumprod_ct, log_1_min_cumprod_ct (T+1 each).
 * t_dev: device int64[B] timesteps; stream_dev: device int64[1] Philox stream id (both read on
 * device so a captured graph can be replayed).  post_dbg: optional [B][K+1][L] log-probabilities.
 * x0_dbg: optional [B][K+1][L] guided log p(x0|xt) (cf_predict_start output). */
typedef struct {
    const float* logits_c;
    const float* logits_u;
    const int64_t* tok_in;
    int64_t* tok_out;
    int B, L, K, T;
    float guidance;
    const float* sched[8];
    const int64_t* t_dev;
    uint64_t seed;
    const int64_t* stream_dev;
    int64_t row0;               /* global row offset of this shard (multi-GPU batch split)   */
    float* post_dbg;
    float* x0_dbg;
    int occupancy;              /* 0 = default; 2 / 3: waves per SIMD the K = 4096 kernel's register budget is sized for       */
                                /* (development switch: the default is 2, no scratch)                                          */
    int post_skip;              /* >= 0; the posterior runs at t' = t - post_skip when t > post_skip, else at t' = t (skip-step */
                                /* sampling, diffusion_transformer.py:700-704); the denoiser's logits are those of step t.     */
                                /* 0 = the plain reverse step                                                                  */
    const uint8_t* known;       /* [B*L], NULL = off (exactly the launch without these fields).  A position with known[pos] != 0   */
                                /* has a given clean token x_known[pos] in [0, K): it reads neither logit row nor tok_in and skips */
                                /* the learned reverse step (frame prediction / interpolation / inpainting); every other position  */
                                /* is sampled as without the mask, bit for bit, from the same uniforms.                            */
    const int64_t* x_known;     /* [B*L]; required when known != NULL, read at known positions only                               */
    int known_mode;             /* 0 renoise: tok_out = Gumbel arg-max of q(x_{t'-1} | x_0 = x_known) (q_pred at level t' - 1,     */
                                /*   wrapped modulo T + 1, t' the posterior's timestep) on the position's own uniforms of the step */
                                /*   -- x_known itself at t' = 0;  1 hold: tok_out = x_known, no uniforms read.                    */
                                /* post_dbg / x0_dbg cannot be combined with known (the masked kernels carry no hooks).            */
                                /* (these three sit before trunc_rate, which stays the struct's last field)                       */
    float trunc_rate;           /* 0 = off, or 0 < r < 1: top-r truncated sampling (VQ-Diffusion's predict_start_with_truncation, */
                                /* "top0.86r").  Of the guided row, class k is kept iff sum_{x_j > x_k} exp(x_j) < r; every other  */
                                /* class drops to -70, without renormalising, before the posterior.  x0_dbg shows the cut row.    */
} gsdd_step_desc;
int gsdd_d3pm_step(const gsdd_step_desc* d, void* stream);

/* Purity-prior reverse step, device half 1 of 2 (p_sample with prior_rule 1 / 2 at t > 0, diffusion_transformer.py:304-326; Improved
 * VQ-Diffusion's high-quality inference).  Per position: log_x_recon = the guided cf_predict_start row exactly as gsdd_d3pm_step
 * computes it (no posterior: that branch drops it), then
 *   score[pos] = exp(max_k log_x_recon)  (prior_rule 2)   or 1  (prior_rule 1)                              -- the RAW score (:316)
 *   smax[b]    = max_l score[b][l]
 *   cand[pos]  = Gumbel arg-max (first index on ties) of `prob` over the K+1 rows, with
 *                prob = log_x_recon                                                        (rule 1, or prior_weight == 0)
 *                prob = log softmax((1 + prior_weight * score / (smax + 1e-10)) * log_x_recon), clamped to [-70, 0]   (rule 2, Eq. 11)
 * The uniforms are the (B, K+1, L) Philox draw of gsdd_d3pm_step at stream stream_dev[0].  Rule 2 with prior_weight > 0 reads the
 * logits twice (scores, smax, draw); otherwise once.  score: float[B*L], smax: float[B], cand: int64[B*L] are outputs that
 * gsdd_d3pm_purity_select consumes.  recon_dbg / prob_dbg: optional [B][K+1][L]; score_dbg: optional [B*L], the normalised score
 * score / (smax + 1e-10) (test hooks, compiled into a separate instantiation). */
typedef struct {
    const float* logits_c;
    const float* logits_u;      /* may be NULL: no guidance                                  */
    int B, L, K;
    float guidance;
    int prior_rule;             /* 1 or 2                                                    */
    float prior_weight;         /* r of Eq. 11, >= 0                                         */
    uint64_t seed;
    const int64_t* stream_dev;
    int64_t row0;               /* global row (position) offset of this shard                */
    float* score;
    float* smax;
    int64_t* cand;
    float* recon_dbg;
    float* prob_dbg;
    float* score_dbg;
    float trunc_rate;           /* 0 = off, or 0 < r < 1: log_x_recon is top-r truncated as in gsdd_step_desc before the score,  */
                                /* `prob` and the draw (recon_dbg shows the cut row; the score keeps its value: the maximum stays) */
} gsdd_purity_desc;
int gsdd_d3pm_purity_step(const gsdd_purity_desc* d, void* stream);

/* Purity-prior reverse step, device half 2 of 2 (:329-346): per sample, reveal n of the [MASK] positions of tok_in, drawn without
 * replacement with weights w_l = score_l / (smax_b + 1e-10) (rule 2) or 1 (rule 1) -- torch.multinomial(_score[i], n) restated as
 * Gumbel-top-n:
 *   key_l = logf(w_l) - logf(-logf(u_l + 1e-30) + 1e-30)   on positions with tok_in == K; the n largest keys win, ties to the lower l;
 *   tok_out[l] = cand[l] there, tok_in[l] elsewhere (tok_out may alias tok_in).
 * u is ONE (B, L) Philox draw at stream stream_dev[0] + stream_add: counter = row * ceil(L / 4) + (l >> 2), word l & 3, where row is the
 * GLOBAL sample index row0 / L + b (row0 as in gsdd_purity_desc, a multiple of L) -- the layout of oracle/philox.py uniform_rows(seed,
 * stream, B, L, row0 / L) -- so the selection does not depend on how a batch is split over lanes or GPUs.
 * n = n_dev[0], read on the device (clamped to [0, L]; when fewer [MASK] positions are left, all of them are revealed and nothing else
 * changes).  L <= 4096 (one sample is sorted in LDS); larger L is GSDD_E_ARG.  key_dbg: optional float[B*L], the keys (test hook). */
typedef struct {
    const int64_t* tok_in;
    int64_t* tok_out;
    const int64_t* cand;
    const float* score;         /* rule 2 only                                               */
    const float* smax;          /* rule 2 only                                               */
    int B, L, K;
    int prior_rule;
    const int64_t* n_dev;
    uint64_t seed;
    const int64_t* stream_dev;
    int64_t stream_add;
    int64_t row0;
    float* key_dbg;
} gsdd_purity_select_desc;
int gsdd_d3pm_purity_select(const gsdd_purity_select_desc* d, void* stream);

/* q_sample for training: tok_out = Gumbel-argmax(q_pred(onehot(x0), t)), diffusion_transformer.py:361-366 */
int gsdd_d3pm_q_sample(const int64_t* x0, int64_t* xt, int B, int L, int K, int T,
                       const float* const* sched, const int64_t* t_dev, uint64_t seed,
                       const int64_t* stream_dev, int64_t row0, void* stream);

/* Forward jump of a state from level a to level b = a + jump (RePaint's resampling: after `jump` reverse steps the chain is diffused
 * forward again and denoised once more), per position and independently, the levels as gsdd_d3pm_step's t: the state the denoiser
 * sees at t is at level t, level -1 is clean and wraps to index T.  With abar / gbar the cumulative schedule (index -1 = T: 1 / 0),
 *   alpha~ = abar_b / abar_a,   1 - gamma~ = (1 - gbar_b) / (1 - gbar_a),   beta~ = (1 - alpha~ - gamma~) / K:
 *   a [MASK] stays [MASK] (no uniforms read); a code i becomes [MASK] with gamma~, stays i with alpha~ + beta~, becomes any other
 *   code with beta~ each -- the product of the one-step matrices of levels a + 1 ... b.
 * The draw is the Gumbel arg-max (first index on ties) over the K + 1 classes on the position's own counters of the (B, K+1, L) Philox
 * draw at stream stream_dev[0], as in gsdd_d3pm_step.  The three log-probabilities are read from `table`, which the host makes in
 * fp64 for this `jump`: row (a mod (T + 1)) holds log(alpha~ + beta~), log(beta~), log(gamma~) as f32. */
typedef struct {
    const int64_t* tok_in;      /* [B*L] tokens in [0, K], K = [MASK]                                                           */
    int64_t* tok_out;           /* [B*L]; may alias tok_in                                                                      */
    int B, L, K, T;
    const float* table;         /* device float[(T + 1) * 3]: (hit, miss, mask) per from-level, the level wrapped modulo T + 1    */
    int jump;                   /* >= 1: the jump `table` was made for (levels a + jump > T - 1 have NaN rows there)            */
    const int64_t* t_dev;       /* device int64[B]: the from-level of every batch row, read on the device, wrapped modulo T + 1 */
    const uint8_t* hold;        /* [B*L] or NULL; non-zero: the position is copied through, no uniforms read                    */
    uint64_t seed;
    const int64_t* stream_dev;  /* device int64[1] Philox stream id                                                             */
    int64_t row0;               /* global row (position) offset of this shard                                                   */
} gsdd_jump_desc;
int gsdd_d3pm_forward_jump(const gsdd_jump_desc* d, void* stream);

/* Composed guidance: several weighted conditions per clip (conjunctions, negative prompts, per-clip weight sweeps) folded into the one
 * logits row a reverse step reads.  A clip has conditions c_0 ... c_{N-1} (1 <= N <= GSDD_COMPOSE_MAX_COND), weights w[b][0 ... N-1]
 * (any finite float, negative allowed) and the null condition u.  Per position and class,
 *   x_i = clamp(log_softmax(logits_i), -70, 0)     i = 0 ... N-1, and x_u likewise (predict_start: the fp64 sum of gsdd_d3pm_step,
 *                                                  the same bits the step computes from the same row)
 *   e   = x_u + sum_i w_i (x_i - x_u)              f32, accumulated in the order i = 0, 1, ...; the first term is the step's own mix,
 *                                                  x_u + w_0 * (x_0 - x_u); no fused multiply-add
 * The reverse step that follows runs with logits_c = e and logits_u = NULL: its log_softmax turns e into clamp(e - logsumexp(e), -70, 0),
 * i.e. cf_predict_start (diffusion_transformer.py:245-247) with the sum over i in place of the single term.
 *   - N = 1, w = s is gsdd_d3pm_step's guided row up to the rounding of the last log-sum-exp (fp64 here, f32 in the two-way kernel):
 *     close to a guided call, not bit-identical to it.
 *   - Weights that sum to 1 cancel x_u: (s, 1 - s) on (caption, negative caption) give x_neg + s (x_cap - x_neg).
 *   - gsdd_step_desc.guidance plays no part: the weights are the scales.  The unconditional row is always needed, also when they sum to 1.
 * `weights` is read on the device, so a captured graph replays whatever the buffer holds at launch.  One launch, no workspace, no
 * memset, no host synchronisation. */
#define GSDD_COMPOSE_MAX_COND 4
typedef struct {
    const float* logits;        /* (n_cond + 1) blocks of [B*L][K] rows: conditions 0 ... n_cond-1, then the null condition (the
                                   order the denoiser leaves for a batch stacked as cat([c_0, ..., c_{N-1}, u])); 16-byte aligned */
    int n_cond, B, L, K;        /* 1 <= n_cond <= 4; K a multiple of 4 in [4, 8192]                                             */
    const float* weights;       /* device float[B][n_cond]                                                                      */
    float* out;                 /* [B*L][K]; may be block 0 of `logits` (out == logits), otherwise it must not overlap `logits` */
} gsdd_compose_desc;
int gsdd_d3pm_compose(const gsdd_compose_desc* d, void* stream);

/* Training objective, forward value: _train_loss + the loss tail of forward (diffusion_transformer.py:391-457, :548)
 * from the denoiser logits of x_t.  Per-position scratch (kl, nll, aux: float[B*L]; x0_recon, xt1_recon: int64[B*L]),
 * per-sample results per_sample[B][4] = (kl_loss, vb_loss, acc rate, keep rate), loss[0] = sum(vb)/(B*L);
 * Lt_history / Lt_count (float[T]) are updated in place (:432-436).  probs: optional [B][K+1][L] = exp(log_model_prob). */
typedef struct {
    const float* logits;        /* [B*L][K] denoiser output for x_t                         */
    const int64_t* x0;          /* (B,L) clean tokens                                       */
    const int64_t* xt;          /* (B,L) noised tokens (gsdd_d3pm_q_sample)                 */
    const int64_t* t_dev;       /* int64[B]                                                 */
    const float* pt;            /* float[B] sampling probability of t                       */
    int B, L, K, T;
    const float* sched[8];
    float mask_weight[2];
    float aux_weight; int adaptive_aux;
    float* kl; float* nll; float* aux; int64_t* x0_recon; int64_t* xt1_recon;
    float* Lt_history; float* Lt_count;
    float* loss; float* per_sample; float* probs;
} gsdd_train_desc;
int gsdd_d3pm_train_loss(const gsdd_train_desc* d, void* stream);

/* dlogits = d loss / d logits of the objective above (backward of predict_start -> q_posterior -> KL / NLL / aux KL). */
int gsdd_d3pm_train_loss_bwd(const gsdd_train_desc* d, float* dlogits, void* stream);
/* Both of the above in ONE pass over the logits (the training step's path; d->probs must be NULL): every output of
 * gsdd_d3pm_train_loss, bit-identical, plus dlogits. */
int gsdd_d3pm_train_loss_grad(const gsdd_train_desc* d, float* dlogits, void* stream);

/* ------------------------------------------------------------------ D3PM training step: backward building blocks
 * (autograd of transformer_utils.py:24-62, 138-159, 258-282, 353-356 and dalle_mask_image_embedding.py:59-79) */
/* out = gelu2(a) (backward=0) or out = du * gelu2'(a) (backward=1), n % 4 == 0 */
int gsdd_gelu2(const float* a, const float* du, float* out, int64_t n, int backward, void* stream);
/* LayerNorm forward of the training step over rows of 64 (nn.LayerNorm / AdaLayerNorm, transformer_utils.py:138-159): stats[row] =
 * (mean, rstd) and y = (x - mean) * rstd * gamma + beta in one pass; gamma/beta = base + sel[row / rows_per_batch] * gstride
 * (sel NULL: one shared pair).  The sampler never materialises y (it is a GEMM prologue there); the training step keeps it as the
 * weight-gradient operand. */
int gsdd_ln_fwd(const float* x, int64_t M, int C, float eps, const float* gamma, const float* beta, const int64_t* sel, int gstride,
                int rows_per_batch, float* stats, float* y, void* stream);
/* LayerNorm backward over rows of 64: dx_out = dx_in + LN'(dh); dgamma/dbeta accumulated (+=) per batch element
 * (acc_by_batch, AdaLN table rows) or globally (affine LN).  gamma = gamma_base + sel[b]*gstride. */
int gsdd_ln_bwd(const float* dh, const float* x, const float* stats, const float* gamma, const int64_t* sel, int gstride,
                int rows_per_batch, int64_t M, int C, const float* dx_in, float* dx_out, float* dgamma, float* dbeta,
                int gacc_stride, int acc_by_batch, void* stream);
/* Process-wide switch of the reductions below (gsdd_ln_bwd's dgamma / dbeta, gsdd_wgrad, gsdd_colsum, gsdd_batch_rowsum,
 * gsdd_d3pm_embed_bwd, gsdd_adaln_bwd's demb): by default workgroups add their partial sums with float atomics, fast, and the last
 * bits of a gradient depend on the order the hardware retires them in.  on != 0: every output address receives the sum of ONE
 * workgroup (or thread) formed in a fixed order -- the same inputs give the same bits -- at the cost of the parallelism over the rows
 * (gsdd_d3pm_embed_bwd walks all rows per table row: for tests and reproducibility runs, not the production shape).  Returns the
 * previous setting.  Read by the host code at launch time: a captured graph keeps the form it was captured with.
 * The six entries and their reproducible forms:
 *   gsdd_wgrad           one workgroup per 64 x 64 output tile walks all ceil(M / 128) row slabs
 *   gsdd_colsum          one block per column group takes all M rows
 *   gsdd_batch_rowsum    one such block per batch element (B launches), each on its own slice of out
 *   gsdd_ln_bwd          one block for the whole call, or with acc_by_batch one single-block launch per batch element
 *   gsdd_d3pm_embed_bwd  a kernel of its own: one thread per (table row or position, column) walks all rows in ascending order
 *   gsdd_adaln_bwd       the first batch element of a timestep adds the shares of all batch elements with that timestep (demb)
 * Two calls silently keep the atomic form with the switch on: gsdd_wgrad, gsdd_colsum and gsdd_ln_bwd with M >= 2^30 rows, and
 * gsdd_ln_bwd with acc_by_batch and M % rows_per_batch != 0 (no whole number of per-batch launches).  The training step reaches
 * neither.  Each form is held to the fast form's fp64 bars and to equal bits from two calls in tests/test_gpu_train_reproducible.py. */
int gsdd_set_deterministic(int on);
/* dW[N][K] += dY^T X (contraction over the M rows), db[N] += column sums of dY (optional) */
int gsdd_wgrad(const float* dY, int ldy, const float* X, int ldx, int64_t M, int N, int K, float* dW, float* db, void* stream);
/* out[n] += sum_m Y[m][n] */
int gsdd_colsum(const float* Y, int ld, int64_t M, int N, float* out, void* stream);
/* out[b][c] = sum_l Y[b*L+l][c] */
int gsdd_batch_rowsum(const float* Y, int B, int L, int C, float* out, void* stream);
/* head-dim-4 self-attention for training: forward that also returns the log2-domain log-sum-exp per (head,row), and the
 * backward (dq|dk|dv rows [M][3*H*4]); scratch: float[H*M].  With a workspace of gsdd_d3pm_attention_workspace_bytes() and
 * L % 32 == 0 the forward runs on the matrix-pipe kernel of gsdd_d3pm_attention; workspace may be NULL (VALU kernel). */
/* mode: GSDD_ATTN_AUTO (= GSDD_ATTN_A8 for L >= 2048, else GSDD_ATTN_P22), GSDD_ATTN_P22 or GSDD_ATTN_A8; anything else is an error. */
int gsdd_d3pm_attention_train(const float* q, const float* k, const float* v, int B, int L, int H, float* out, float* lse,
                              void* workspace, int64_t workspace_bytes, int mode, void* stream);
/* With a workspace of gsdd_d3pm_attention_bwd_workspace_bytes() and L % 32 == 0 the backward runs on the bf16 matrix pipe
 * (pre-split operand images, dQ kernel + dK/dV kernel); otherwise on the VALU kernels, which need `scratch`. */
int64_t gsdd_d3pm_attention_bwd_workspace_bytes(int B, int L, int H);
/* variant: GSDD_ATTN_BWD_AUTO = the fused kernel (one pass over the scores for dQ, dK and dV); GSDD_ATTN_BWD_VALU = the vector
 * kernels whatever the shape; the rest are development variants kept as cross-checks of each other (tests/test_gpu_training.py):
 * _SPLIT = dQ kernel + dK/dV kernel, _FQC64 / _FQC128 = queries per LDS chunk of the fused kernel (default 96), _NW8 = eight waves
 * per workgroup, _DBG1 / _DBG2 = the fused kernel stopping after its dQ / dK stage. */
#define GSDD_ATTN_BWD_AUTO 0
#define GSDD_ATTN_BWD_VALU 1
#define GSDD_ATTN_BWD_SPLIT 2
#define GSDD_ATTN_BWD_FQC64 3
#define GSDD_ATTN_BWD_FQC128 4
#define GSDD_ATTN_BWD_NW8 5
#define GSDD_ATTN_BWD_DBG1 6
#define GSDD_ATTN_BWD_DBG2 7
#define GSDD_ATTN_BWD_DEV_LAST 7
int gsdd_d3pm_attention_bwd(const float* q, const float* k, const float* v, const float* o, const float* dO, const float* lse,
                            int B, int L, int H, float* dqkv, float* scratch, void* workspace, int64_t workspace_bytes,
                            int variant, void* stream);
/* demb[tok] += dx, dpos[l] += dx */
int gsdd_d3pm_embed_bwd(const float* dx, const int64_t* tok, int B, int L, int D, int n_embed, float* demb, float* dpos,
                        void* stream);
/* y = W x + b over R rows: dx (optional) = dy W ; dW += dy^T x ; db (optional) += sum dy */
int gsdd_small_linear_bwd(const float* dy, const float* x, const float* w, int R, int Cin, int Cout, float* dx, float* dw,
                          float* db, void* stream);
/* backward of gsdd_adaln_table restricted to the rows t[b]: dtab [B][2D] -> demb (+=, rows t[b]), dW (+=), db (+=) */
int gsdd_adaln_bwd(const float* dtab, const int64_t* t, int B, int D, const float* emb, const float* w, float* demb, float* dw,
                   float* db, void* stream);
/* torch.optim.Adam update (no weight decay), step >= 1, over many tensors in one launch: table[b] = {p, g, m, v, n} (device pointers
 * as int64, n <= 4096 elements) for block b; the caller chops every parameter into such chunks. */
int gsdd_adam_multi(const int64_t* table, int n_blocks, float lr, float beta1, float beta2, float eps, int step, void* stream);
/* ... with the step count (>= 1) read from device memory at execution time: the form a captured, replayed training step uses (the
 * caller sets *step_dev before each replay, or advances it with gsdd_advance inside the graph). */
int gsdd_adam_multi_dev(const int64_t* table, int n_blocks, float lr, float beta1, float beta2, float eps, const int64_t* step_dev,
                        void* stream);

/* ------------------------------------------------------------------ optimiser stage: gradient norm, clip, AdamW, EMA, non-finite skip
 * Three launches per step whatever the number of parameters, over a WIDE block table: table[b] = {p, g, m, v, n, e, flags} (7 int64;
 * device pointers as int64, 1 <= n <= 4096 elements of one tensor; e: the tensor's running average or 0; flags bit 0
 * (GSDD_OPTIM_DECAYS): the tensor takes weight decay).  p and g need 4-byte alignment only (16-byte aligned ones are read four wide);
 * m, v and e are 16-byte aligned at every block.  Everything that changes from step to step lives in the device state block, so the
 * three launches are the same graph nodes in a launch-by-launch step and in a captured, replayed one.  The caller writes `step`
 * (>= 1, the count of THIS update) and `lr` before the stage; gsdd_grad_norm_finalize writes the other words.  A state block that
 * never went through finalize must hold clip_coef = 1, finite = 1.
 * The gradient buffers are NEVER rewritten: the update applies the clip coefficient to the gradients it reads, g itself keeps the
 * unclipped values; the norm and the coefficient are available to the caller as the device scalars state->grad_norm / clip_coef. */
#define GSDD_OPTIM_DECAYS 1
typedef struct {
    int64_t step;             /* caller: the step count of this update, >= 1 (bias corrections, EMA warm-up)                          */
    int64_t skipped_steps;    /* finalize: += 1 whenever skip_nonfinite is on and the norm is inf / NaN                               */
    float lr;                 /* caller: this step's learning rate                                                                    */
    float grad_norm;          /* finalize: the global L2 norm of the gradients                                                        */
    float clip_coef;          /* finalize: min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_); 1 without clipping      */
    int32_t finite;           /* finalize: 0 iff skip_nonfinite is on and the norm is inf / NaN -- the update then writes nothing     */
} gsdd_optim_state;
/* partials[b] = sum of g^2 over block b, accumulated in double (the square of an f32 is exact in double); one workgroup per block,
 * no atomics, a fixed order: the same inputs give the same bits. */
int gsdd_grad_sqnorm(const int64_t* table, int n_blocks, double* partials, void* stream);
/* One workgroup: sums partials[0 .. n_blocks) in a fixed order in double and writes grad_norm, clip_coef, finite and skipped_steps.
 * max_norm > 0; +infinity means "no clipping" (clip_coef = 1).  skip_nonfinite == 0: finite is always 1 and nothing is counted (a
 * non-finite norm then poisons the update exactly as torch's clip_grad_norm_ + AdamW would). */
int gsdd_grad_norm_finalize(const double* partials, int n_blocks, float max_norm, int skip_nonfinite, gsdd_optim_state* state,
                            void* stream);
/* The update, one workgroup per block; step, lr, clip_coef and finite are read from *state.  finite == 0: nothing is written.
 * Otherwise with g' = clip_coef g:  p <- p (1 - lr weight_decay) for tensors with GSDD_OPTIM_DECAYS (torch.optim.AdamW: decay first),
 * then gsdd_adam_multi_dev's arithmetic on g' in its operation order, every operation in f32 and rounded once (the library is built
 * without contraction):  m <- beta1 m + (1 - beta1) g' ;  v <- beta2 v + ((1 - beta2) g') g' ;
 * p <- p - (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps)), with the bias corrections bc_i = (float)(1 - pow((double)beta_i, (double)step))
 * evaluated in double per workgroup; then where e != 0
 * e <- d e + (1 - d) p_new with d = min(ema_decay, (1 + step) / (10 + step)) evaluated in double per workgroup.
 * With clip_coef = 1, no flag and e = 0 the words written are gsdd_adam_multi_dev's, bit for bit: the two extra products are by 1.f
 * (tests/golden/adam_plain_bits.npz holds that kernel's words).
 * weight_decay >= 0, 0 <= ema_decay < 1 (read only where a block has an e). */
int gsdd_adamw_ema_multi(const int64_t* table, int n_blocks, float beta1, float beta2, float eps, float weight_decay, float ema_decay,
                         const gsdd_optim_state* state, void* stream);
/* Exchanges p and e of every block that has an e, exactly (the averaged weights in and out of the model, one launch). */
int gsdd_swap_multi(const int64_t* table, int n_blocks, void* stream);

/* ------------------------------------------------------------------ classifier-free training: condition dropout, learned null embedding
 * (the reference substitutes empty_text_embed for the condition at diffusion_transformer.py:541-543) */
/* out[b] = drop_b ? null_rows : cond[b] over (Te, C) rows, drop_out[b] = drop_b.  drop_b = drop_in[b] != 0 when drop_in is given,
 * else u_b < p with u_b = (w >> 8) * 2^-24, w = word 0 of Philox4x32-10 with key `seed` and counter (row0 + b [64 bit], sid[0], 1):
 * every other draw of the library has 0 in counter word 3.  cond / out: [B][Te][C]; null_rows: [Te][C]; sid: device int64[1], the
 * stream id of the step's q_sample draw (may be NULL with drop_in); drop_in / drop_out: B bytes.  C % 4 == 0, 1 <= Te <= 77,
 * 0 <= p <= 1, rows 16-byte aligned; out must not overlap cond or null_rows. */
int gsdd_cond_dropout(const float* cond, const float* null_rows, int B, int Te, int C, float p, uint64_t seed, const int64_t* sid,
                      int64_t row0, const uint8_t* drop_in, float* out, uint8_t* drop_out, void* stream);
/* dnull[j][:] += sum_{b: drop[b]} (dk[b][j][:] Wk + dv[b][j][:] Wv) for j < Te: the gradient of the null rows through one block's
 * attn2.key / attn2.value.  dk / dv: [B][Te][D]; wk / wv: [D][C]; dnull: [Te][C]; dk and wk may both be NULL (one condition token: no
 * key term).  Samples in ascending b, features in ascending d, no atomics: bitwise reproducible.  With no sample dropped dnull is not
 * written.  1 <= Te <= 77, 1 <= D <= 4096. */
int gsdd_cond_null_grad(const float* dk, const float* dv, const uint8_t* drop, const float* wk, const float* wv, int B, int Te, int D,
                        int C, float* dnull, void* stream);

/* t[b] += dt ; stream[0] += ds   (device-side loop counters for the captured step graph) */
int gsdd_advance(int64_t* t_dev, int B, int64_t dt, int64_t* stream_dev, int64_t ds, void* stream);
/* t[b] = max(t[b] + dt, t_min) ; stream[0] += ds   (the skip-step sampler's counter: t moves by -(1 + s) and stops at 0) */
int gsdd_advance_floor(int64_t* t_dev, int B, int64_t dt, int64_t t_min, int64_t* stream_dev, int64_t ds, void* stream);

/* The purity chain's counter: step[0] += 1; i = min(step[0], n_calls - 1); t[b] = plan_t[i] (b < B); n[0] = plan_n[i]; stream[0] += ds.
 * plan_t / plan_n: device int64[n_calls], the (t, n) of every purity call (d3pm.purity_plan); placed after a call inside the captured
 * graph it loads the next call's timestep and reveal count, so that one graph replays the whole chain. */
int gsdd_advance_plan(int64_t* step_dev, const int64_t* plan_t, const int64_t* plan_n, int64_t n_calls, int64_t* t_dev, int B,
                      int64_t* n_dev, int64_t* stream_dev, int64_t ds, void* stream);

/* ------------------------------------------------------------------ long clips: sliding-window rollout and stitched decode
 * A long grid of n latent frames is sampled as windows of F frames that overlap by k (stride s = F - k): window w covers long frames
 * [w s, w s + F) and is conditioned on the last k frames of window w - 1; long frame f takes its tokens from the first window that
 * sampled it (window 0: f < F; window w >= 1: f in [w s + k, w s + F)); frames >= n are dropped.
 *
 * gsdd_d3pm_window_slide: the op between two windows, one launch, on the caller's fixed buffers (safe to capture: every fill is a
 * store of the kernel).  tok[Bs][F hw] holds finished window w = state[0]:
 *   long_tok[b][(w s + f) hw + q] = tok[b][f hw + q] for the frames f the window contributes whose long frame is < n (long_tok: the
 *       caller's first row of the (B, n hw) long buffer, row pitch n hw; nothing is written behind a row's end);
 *   x_known[b][: k hw] = tok[b][s hw :]; bad[0] += the number of those tokens outside [0, K) ([MASK] = K is no clean token);
 *   known[b][p] = p < k hw; tok[b][p] = K; t2[i] = t0 for i < n_t2; state[0] = w + 1.
 * state: device int64[2], {the finished window's index, 0}; the second word is the kernel's own arrival counter and is 0 again when
 * the launch has finished.  The entry point is not idempotent: every launch moves state[0] on, so the caller zeroes the state at the
 * start of every rollout and does not reuse it after a failed launch.  A state[0] outside [0, n] writes nothing to long_tok (x_known,
 * known, tok and t2 are rewritten all the same).  final_copy = 1 (behind the last window): only the
 * copy to long_tok; x_known, known, t2 and bad may be null and the state does not move.
 * GSDD_E_ARG before the launch for a null pointer, sizes below 1, k outside [1, F - 1], n < F, K < 1, t0 < 0, n_t2 outside
 * [0, Bs F hw], Bs F hw of 2^31 or more.
 *
 * gsdd_clip_window_blend: one decoded window win[BC][Fw][HW] (BC = batch x channels planes) merged into the long clip
 * out[BC][Fo][HW] at output frame f0.  Frames f0 + j >= Fo are not written.  The first n_ov frames of the window overlap frames
 * the window before has written: GSDD_BLEND_LINEAR crossfades them in fp32, out <- out + a_j (win - out) with
 * a_j = (j + 1) / (n_ov + 1); GSDD_BLEND_KEEP leaves them as they are (no write); GSDD_BLEND_REPLACE overwrites them.  The frames
 * behind the overlap are copied bit for bit.
 * GSDD_E_ARG before the launch for a null pointer, sizes below 1, BC above 65535, Fo < Fw, n_ov outside [0, Fw - 1], f0 outside
 * [0, Fo - 1], n_ov > 0 with f0 = 0, an unknown mode, a pointer off 4-byte alignment. */
#define GSDD_BLEND_LINEAR 0
#define GSDD_BLEND_KEEP 1
#define GSDD_BLEND_REPLACE 2
int gsdd_d3pm_window_slide(int64_t* tok, int64_t* long_tok, int64_t* x_known, uint8_t* known, int64_t* t2, int64_t* state, int* bad,
                           int Bs, int F, int hw, int k, int n, int K, int64_t t0, int n_t2, int final_copy, void* stream);
int gsdd_clip_window_blend(const float* win, float* out, int BC, int Fw, int HW, int Fo, int f0, int n_ov, int mode, void* stream);

/* uniform Philox floats, layout of oracle/philox.py uniform_rows (test hook) */
int gsdd_philox_uniform(uint64_t seed, int64_t stream_id, int64_t row0, int64_t n_rows, int n_cols,
                        float* out, void* stream);

/* ------------------------------------------------------------------ CLIP text tower (text-conditioned sampling)
 * The three pieces of clip.model.CLIP.encode_text (called by the reference at src/models/text_models/clip_text_embedding.py:56-65)
 * that are not a gsdd_gemm / gsdd_row_stats call (csrc/text_tower.hip; the attention is csrc/clip_attention.hip, one kernel template
 * for both CLIP towers); gif-synthesis-with-discrete-diffusion_amd/text.py strings the tower together.
 * `ids_host` / `eot_host` are the one exception to "every pointer is a device pointer": an optional HOST copy of the same integers
 * (the tokenizer produces them on the host).  When given, every value is range-checked before anything is launched and an
 * out-of-range one returns GSDD_E_ARG; without it (NULL) the kernels still never read out of range: the offending output row is
 * NaN. */
/* x[b][s][:] = tok_emb[ids[b][s]] + pos_emb[s] for s < S   (encode_text: token_embedding(text) + positional_embedding).
 * ids: int64 [B][ids_pitch] (the first S of each row are used), tok_emb [vocab][C], pos_emb [n_pos][C], x rows [B*S][C];
 * 1 <= S <= 77, S <= n_pos, C % 4 == 0. */
int gsdd_text_embed(const int64_t* ids, const int64_t* ids_host, int B, int S, int ids_pitch, int C, const float* tok_emb, int vocab,
                    const float* pos_emb, int n_pos, float* x, void* stream);
/* Causal multi-head self-attention over fused rows qkv[B*S][3C] = (q | k | v), head h at columns h*d of each third, d = C / n_head
 * in {64, 32, 16} (ViT-B/32's and ViT-L/14's towers have d = 64; the narrow ones serve small test towers); out rows [B*S][C] = softmax(scale q k^T + causal mask) v; 1 <= S <= 77.  Exact-f32 matrix instructions
 * (v_mfma_f32_16x16x4_f32); key tiles above the diagonal are never computed.
 * Replaces the nn.MultiheadAttention of every ResidualAttentionBlock under encode_text's build_attention_mask. */
int gsdd_text_attention(const float* qkv, int B, int S, int C, int n_head, float scale, float* out, void* stream);
/* out[b][:] = x[b*S + eot[b]][:]   (encode_text: x[arange(B), text.argmax(-1)]; the final LayerNorm is per row, so it and the
 * projection then run on these B rows).  eot: int64 [B], each in [0, S). */
int gsdd_text_pool(const float* x, const int64_t* eot, const int64_t* eot_host, int B, int S, int C, float* out, void* stream);

/* ------------------------------------------------------------------ CLIP image tower (CLIPSIM in the evaluator)
 * The three pieces of clip.model.VisionTransformer / transformers.CLIPVisionModelWithProjection that are not a gsdd_gemm /
 * gsdd_row_stats / gsdd_ln_apply / gsdd_text_pool call (csrc/clip_vision.hip; the attention is csrc/clip_attention.hip);
 * gif-synthesis-with-discrete-diffusion_amd/vision.py strings the tower together.  Every pointer is a device pointer. */
/* clips[B][3][T][H][W] f32, ImageNet-normalised (what the decoder returns and the evaluator receives) -> patch rows
 * out[B*T*G*G][3*P*P], G = R / P: row (b*T + t)*G*G + gy*G + gx holds the patch's pixels in the order [c][py][px] of a
 * Conv2d(3, C, P, stride P) weight flattened to [C][3*P*P], so the patch embedding is one plain gsdd_gemm linear.
 * Per pixel, in this order: undo the ImageNet mean / std; quantise to a uint8 level as the evaluator does ((x*255) truncated and
 * clamped to 0..255, kept as level / 255); bicubic resize to R x R; clamp to [0, 1]; normalise with CLIP's mean (0.48145466,
 * 0.4578275, 0.40821073) and std (0.26862954, 0.26130258, 0.27577711).
 * The resize is TORCH's bicubic -- F.interpolate(mode="bicubic", align_corners=False, antialias=False): Keys' kernel with
 * a = -0.75, border indices clamped -- and NOT PIL's (a = -0.5, fixed-point weights, antialiasing), which the `clip` package's
 * preprocessing uses: parity with that preprocessing is not claimed.  H == W <= R <= 4096 and R % P == 0, anything else is
 * GSDD_E_ARG (non-square or shrunk frames would need PIL's crop / antialiasing).  At H == R the result is the quantised frame. */
int gsdd_clip_frame_patches(const float* clips, int B, int T, int H, int W, int R, int P, float* out, void* stream);
/* x[n][0][:] = class_emb + pos[0],  x[n][1 + p][:] = patches[n*(S-1) + p][:] + pos[1 + p]   (the class token in FRONT of the
 * patches, then the position embedding).  patches rows [N*(S-1)][C] (the patch gemm's output), class_emb [C], pos [S][C],
 * x rows [N*S][C]; S = G*G + 1, 1 <= S <= 77, C % 4 == 0, rows 16-byte aligned. */
int gsdd_clip_vision_embed(const float* patches, const float* class_emb, const float* pos, int N, int S, int C, float* x, void* stream);
/* NON-causal multi-head self-attention over fused rows qkv[B*S][3C] = (q | k | v), head h at columns h*d of each third,
 * d = C / n_head in {64, 32, 16}; out rows [B*S][C] = softmax(scale q k^T) v; 1 <= S <= 77 (ViT-B/32 at 224: S = 50; ViT-B/16 and
 * ViT-L/14 have longer sequences and are out of range).  The contract, the layout and the kernel template of gsdd_text_attention
 * (csrc/clip_attention.hip; exact-f32 matrix instructions, v_mfma_f32_16x16x4_f32) with every query seeing every key: the keys of the last 16-key tile at positions >= S are
 * masked before the row maximum and the sum. */
int gsdd_clip_attention(const float* qkv, int B, int S, int C, int n_head, float scale, float* out, void* stream);

/* ------------------------------------------------------------------ GIF export of decoded clips (gif.py; csrc/gif.hip, csrc/gif_refine.hip, csrc/gif_delta.hip, csrc/gif_host.hpp)
 * Colour quantisation on the device, median cut and the GIF89a / LZW writer on the host.  clips[B][3][T][H][W] f32 are the decoder's
 * ImageNet-normalised clips.  Each pixel's uint8 channels are formed by the evaluator's rule: v = (x*std[c] + mean[c]) * 255 in fp32
 * in that order, clamped to [0, 255] (NaN -> 0), truncated.  Everything after that step is integer arithmetic with integer atomics:
 * every output below is exact and does not depend on the order the workgroups run in.  A "group" shares one palette: one clip
 * (per_frame = 0, G = B) or one frame (per_frame = 1, G = B*T).  H, W <= 65535 and at most 2^24 pixels per group (so that no box sum
 * overflows 32 bits), anything else is GSDD_E_ARG before any launch. */
/* hist[G][32768] uint32 (zeroed by the call): pixels per bin, bin = (r>>3)<<10 | (g>>3)<<5 | (b>>3). */
int gsdd_gif_histogram(const float* clips, int B, int T, int H, int W, int per_frame, uint32_t* hist, void* stream);
/* box_of_bin[G][32768] uint8 (device, 16-byte aligned; gsdd_gif_median_cut's table) -> sums[G][256][4] uint32 (zeroed by the call): per
 * box the pixel count and the sums of the R, G and B uint8 values.  A palette colour is the rounded mean (2*sum + count) / (2*count). */
int gsdd_gif_box_sums(const float* clips, int B, int T, int H, int W, int per_frame, const uint8_t* box_of_bin, uint32_t* sums,
                      void* stream);
/* palette[G][256][4] uint8 (R, G, B, unused; 4-byte aligned), n_colors[G] int32 (device) -> out[B][T][H][W] uint8: per pixel the index
 * among entries 0 .. n_colors-1 with the smallest integer squared RGB distance, the lowest index on ties.  dither is an amplitude in
 * 0 .. 64 (0 = off): every channel first gets the ordered-dither offset ((M[y&7][x&7] * dither) >> 6) - (dither >> 1) and is clamped
 * to [0, 255]; M is the 8 x 8 Bayer matrix M(x,y) = sum_{i=0..2} ((((x>>i)^(y>>i))&1) << (2*(2-i)+1) | ((y>>i)&1) << (2*(2-i))). */
int gsdd_gif_map(const float* clips, int B, int T, int H, int W, int per_frame, const uint8_t* palette, const int32_t* n_colors, int dither,
                 uint8_t* out, void* stream);
/* One assignment pass of a k-means (Lloyd) refinement (csrc/gif_refine.hip).  palette, n_colors as gsdd_gif_map takes them ->
 * sums[G][256][4] uint32: per entry i < n_colors the count and the R, G, B sums of the pixels whose nearest entry is i -- nearest exactly
 * as in gsdd_gif_map without dither: integer squared distance, the lowest index on ties, so the higher of two equal entries stays empty --
 * and sse[G] uint64 (8-byte aligned): the group's total squared distance to the nearest entries (64 bits: 3 * 255^2 * 2^24 > 2^32).  Both
 * are zeroed by the call; with n_colors[g] <= 0 they stay 0.  The next palette of the refinement is the rounded mean
 * (2*sum + count) / (2*count) of every entry with count > 0. */
int gsdd_gif_palette_sums(const float* clips, int B, int T, int H, int W, int per_frame, const uint8_t* palette, const int32_t* n_colors,
                          uint32_t* sums, uint64_t* sse, void* stream);
/* Floyd-Steinberg error diffusion (csrc/gif_refine.hip): palette, n_colors as gsdd_gif_map takes them -> out[B][T][H][W] uint8.  Every
 * frame starts with no error, and errors outside the frame are 0: nothing is carried from frame to frame.  Pixels are visited left to
 * right, rows top to bottom (no serpentine).  With e_c(y,x) the error of channel c left at pixel (y,x),
 *   acc      = 7*e_c(y,x-1) + 3*e_c(y-1,x+1) + 5*e_c(y-1,x) + 1*e_c(y-1,x-1)
 *   target_c = clamp(level_c + ((acc + 8) >> 4), 0, 255)          (>>: arithmetic, i.e. floor((acc + 8) / 16); level_c: the uint8 rule)
 *   index    = the entry among 0 .. n_colors-1 nearest to target, as in gsdd_gif_map: integer squared distance, lowest index on ties
 *   e_c(y,x) = target_c - palette[index]_c
 * With n_colors[g] <= 0 the index is 0, as in gsdd_gif_map.  The result is exact and does not depend on how the kernel schedules the
 * pixels (one workgroup per frame, one thread per row, each row two pixels behind the row above). */
int gsdd_gif_diffuse(const float* clips, int B, int T, int H, int W, int per_frame, const uint8_t* palette, const int32_t* n_colors,
                     uint8_t* out, void* stream);
/* The delta stage between the quantiser and gsdd_gif_encode_delta (csrc/gif_delta.hip).  indices[B][T][H][W] uint8 from gsdd_gif_map or
 * gsdd_gif_diffuse (any dither), palette and n_colors as gsdd_gif_map takes them, tolerance an integer squared RGB distance in
 * 0 .. 195075 (3 * 255^2) -> out[B][T][H][W] uint8 (not `indices` itself), rects[B][T][4] int32 = x0, y0, x1, y1 inclusive,
 * changed[B][T] uint32; rects and changed are initialised by the call.  The rule, for every pixel of the canvas on its own, with
 * `shown` the RGB the pixel displays, for t = 0 .. T-1 and g the frame's group:
 *   transparent(g) = n_colors[g] < 256 ? n_colors[g] : -1
 *   c         = palette[g][indices_t]  (R, G, B)
 *   level_t   = the uint8 rule of the pixel in frame t (no dither offset)
 *   unchanged = t > 0 && (c == shown || (tolerance > 0 && transparent(g) >= 0 && d2(level_t, shown) <= tolerance))
 *               (d2: the integer squared RGB distance of gsdd_gif_map)
 *   out_t     = unchanged && transparent(g) >= 0 ? transparent(g) : indices_t
 *   shown     = unchanged ? shown : c
 * rects[b][t] is the bounding box of the pixels of frame t that are not unchanged -- all of frame 0; (W, H, -1, -1) for a frame without
 * any -- and changed[b][t] their number.  What follows from the rule:
 *   - colours are compared, not indices: duplicated palette entries and per-frame palettes behave;
 *   - the tolerance compares a pixel with what is DISPLAYED, not with its level in the frame before: a slow drift is repainted once it
 *     has left the tolerance, it does not creep away;
 *   - with tolerance = 0 a file written from out, rects and transparent() by gsdd_gif_encode_delta decodes to exactly the frames of the
 *     file gsdd_gif_encode writes from indices.  A group with 256 colours has no free index: its frames are cropped only.
 * With tolerance = 0 `clips` is not read.  Exact, and independent of the order the workgroups run in. */
int gsdd_gif_delta(const float* clips, const uint8_t* indices, int B, int T, int H, int W, int per_frame, const uint8_t* palette,
                   const int32_t* n_colors, int tolerance, uint8_t* out, int32_t* rects, uint32_t* changed, void* stream);
/* The entries below are HOST code on HOST pointers: nothing is launched, no stream. */
/* Deterministic integer median cut of one histogram into at most `colors` (2 .. 256) boxes: start with one box of every occupied bin;
 * split the box with the largest pixel count among those with more than one occupied bin (ties: lowest index) along its axis of largest
 * extent in bin coordinates (ties R, G, B), after the first plane where twice the cumulative count reaches the box total (one plane
 * earlier if that is the last plane); the lower part keeps the index, the upper part is appended; stop when no box can be split.
 * box_of_bin[32768]: the box of each occupied bin, 255 for an unoccupied one; *n_boxes: the boxes made (0 for an empty histogram). */
int gsdd_gif_median_cut(const uint32_t* hist, int colors, uint8_t* box_of_bin, int* n_boxes);
/* A buffer size that always holds the file of T frames of H x W. */
int64_t gsdd_gif_encode_bound(int T, int H, int W);
/* GIF89a file of indices[T][H][W] -> out[0 .. return value).  palettes[n_palettes][256][3] uint8 with n_colors[n_palettes] in 1 .. 256:
 * n_palettes = 1 is a global colour table, n_palettes = T one local table per frame; tables are padded with zeros to a power of two
 * of at least 2 entries.  delay_cs: centiseconds per frame, loop: NETSCAPE2.0 loop count (0 = for ever), both 0 .. 65535.  One graphic
 * control extension per frame (disposal 1), LZW with minimum code size max(2, bits), a clear code first and again whenever the table
 * holds 4096 entries; whole frames, no transparency (delta frames: gsdd_gif_encode_delta).  *clear_codes (may be NULL): the clear codes written, all frames.
 * Returns the byte count; GSDD_E_ARG for bad arguments (an index outside its table included); GSDD_E_CAP when cap is too small --
 * nothing is written at or behind out[cap] in any case. */
int64_t gsdd_gif_encode(const uint8_t* indices, int T, int H, int W, const uint8_t* palettes, const int32_t* n_colors, int n_palettes,
                        int delay_cs, int loop, uint8_t* out, int64_t cap, int64_t* clear_codes);
/* gsdd_gif_encode for delta frames: frame t is written as the sub-image rects[t] = x0, y0, x1, y1 (inclusive) of the full-frame
 * indices[T][H][W] (gsdd_gif_delta's out), its rows read at stride W; the empty marker (W, H, -1, -1) is written as the 1 x 1 image at
 * (0, 0).  transparent[n_palettes]: the transparent index of each table's frames, -1 = none: the graphic control extension carries the
 * flag and the index (disposal 1), and the table covers the index -- max(n_colors, transparent + 1) entries, then padded to the power
 * of two, from which the minimum code size follows.  The LZW writer is gsdd_gif_encode's and gsdd_gif_encode_bound bounds the result.
 * With whole-frame rectangles and no transparent index the bytes are gsdd_gif_encode's.  GSDD_E_ARG as gsdd_gif_encode, and for a
 * rectangle that leaves the canvas or is inverted (other than the empty marker), a transparent index outside -1 .. 255, and an index
 * inside a rectangle that is neither below n_colors nor the transparent one; GSDD_E_CAP when cap is too small -- nothing is written at
 * or behind out[cap] in any case. */
int64_t gsdd_gif_encode_delta(const uint8_t* indices, int T, int H, int W, const uint8_t* palettes, const int32_t* n_colors,
                              int n_palettes, const int32_t* rects, const int32_t* transparent, int delay_cs, int loop, uint8_t* out,
                              int64_t cap, int64_t* clear_codes);

/* ------------------------------------------------------------------ GIF import (gif.py; csrc/gif_read.hip, csrc/gif_read_host.hpp)
 * The host walks the file and decodes the LZW streams; the device composites the frame rectangles (transparency, disposal) onto the
 * canvas and expands palette indices to RGB.  Tables are plain integers, no struct: frames[F][8] int32 = x, y, w, h, raster offset,
 * palette row, transparent index (-1 = none), disposal (0 .. 3; 4 .. 7 are stored as 0); palettes[P][256][4] uint8 (R, G, B, 0 -- the
 * layout of gsdd_gif_map; zeros behind a table's size), the global table first if there is one, then the local ones in file order.
 * The first two entries are HOST code on HOST pointers reading FOREIGN bytes: nothing is launched, no stream; they never read outside
 * data[0 .. n).  Malformed input -- a bad signature, an empty canvas, an image that leaves the canvas or has w = 0 or h = 0, an image
 * without any colour table, a minimum code size outside 1 .. 8, an unknown block, no frames, an LZW code above the next free table
 * entry, a first code after a clear code that is not a literal, data that ends before w*h pixels, a sub-block chain cut off by the end
 * of the data -- is GSDD_E_ARG with gsdd_last_error() naming the byte offset.  A missing trailer behind a complete frame is accepted. */
/* Block structure only, no LZW.  info[8]: W, H, frames F, colour tables P (global + local), raster bytes (the sum of w*h over the
 * frames), NETSCAPE2.0 loop count (-1 if absent), 1 if a global table exists, the version (87 or 89). */
int gsdd_gif_probe(const uint8_t* data, int64_t n, int64_t* info);
/* frames[F][8], delays[F] (centiseconds; 0 for a frame without a graphic control extension), palettes[P][256][4] and raster (the
 * decoded indices of every frame rectangle back to back, rows in DISPLAY order: interlacing is undone) with F, P of gsdd_gif_probe on
 * the same bytes.  LZW: clear and end codes, KwKwK, a deferred clear (with 4096 entries the table stops growing and codes stay 12
 * bits), sub-blocks of 1 .. 255 bytes; decoding of a frame stops at w*h pixels.  GSDD_E_CAP when the frames hold more than raster_cap
 * (or more than 2^31 - 1) pixels: nothing is written at or behind raster[raster_cap] in any case. */
int gsdd_gif_decode(const uint8_t* data, int64_t n, int32_t* frames, int32_t* delays, uint8_t* palettes, uint8_t* raster,
                    int64_t raster_cap);
/* Device: raster, frames[F][8], palettes (4-byte aligned) as gsdd_gif_decode wrote them, select[T_out] int32 -> out[T_out][H][W][3]
 * uint8, the input of gsdd_preprocess_clip.  Per pixel, starting from the matte (0xRRGGBB), for f = 0 .. select[T_out-1]:
 *   1. f > 0: frame f-1's disposal inside frame f-1's rectangle: 2 sets the pixel to the matte (not the logical screen's background
 *      colour), 3 to the value saved in step 2 of frame f-1, 0 and 1 leave it;
 *   2. if frame f has disposal 3 the pixel's value is saved;
 *   3. inside frame f's rectangle an index other than f's transparent index sets the pixel to palettes[row_f][index];
 *   4. the pixel is written to every slot k with select[k] == f.
 * select is non-decreasing in 0 .. F-1 and may repeat a frame (a short clip padded with its last frame).  select_host[T_out] is the
 * HOST copy of select: the call checks it before anything is launched and reads the last frame to walk from it (the library never
 * reads device memory on the host).  A select_host that decreases or leaves 0 .. F-1, W or H outside 1 .. 65535, T_out < 1, F < 1 or
 * a matte outside 0 .. 0xFFFFFF is GSDD_E_ARG.  One launch; every byte of out is written. */
int gsdd_gif_compose(const uint8_t* raster, const int32_t* frames, const uint8_t* palettes, int F, int W, int H, const int32_t* select,
                     const int32_t* select_host, int T_out, int matte_rgb, uint8_t* out, void* stream);

/* ------------------------------------------------------------------ paired video metrics (metrics.py; csrc/paired_metrics.hip)
 * Squared error and SSIM of two clips, per (clip, frame, channel) plane, on their uint8 levels.  The operands a and b share B, T, H, W;
 * each is, on its own, in one of two forms:
 *   form 0   float32 planar [B][3][T][H][W], ImageNet-normalised as the decoder returns it; a level is the uint8 rule of the GIF export
 *            above: v = (x*std[c] + mean[c]) * 255 in fp32 in that order, truncated, clamped to [0, 255], NaN -> 0;
 *   form 1   uint8 interleaved [B][T][H][W][3] (gsdd_gif_compose's out, palette[indices]); a level is the byte.
 * SSE    sse[b][t][c] = sum over y, x of (a - b)^2 on the levels: an exact integer.
 * SSIM   (Wang et al. 2004, per channel, "valid" windows, data range 255)
 *   window   w[i][j] = g[i] g[j], g[i] ~ exp(-(i - 5)^2 / (2 * 1.5^2)) for i = 0 .. 10, normalised in fp64 and THEN rounded to fp32;
 *            these eleven fp32 values, widened again, are the rule (g[10 - i] = g[i]):
 *              g[0..5] = 0x1.0d956cp-10, 0x1.f1fe02p-8, 0x1.26eb18p-5, 0x1.bff0fep-4, 0x1.b43c4p-3, 0x1.10656p-2
 *   positions every window with its corner at 0 <= y <= H - 11, 0 <= x <= W - 11: (H - 10)(W - 10) of them, no padding
 *   moments  mu_a, mu_b the weighted means sum w a, sum w b; var_a, var_b, cov the weighted second moments about them
 *            sum w (a - mu_a)^2, sum w (b - mu_b)^2, sum w (a - mu_a)(b - mu_b).  Nothing is divided by sum w = 1 - 2.8e-9, so
 *            sum w (a - mu_a)^2 = sum w a a - (2 - sum w) mu_a^2: at mu = 255 the factor moves s by 3e-6, it is part of the rule
 *   C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2
 *   s        = (2 mu_a mu_b + C1)(2 cov + C2) / ((mu_a^2 + mu_b^2 + C1)(var_a + var_b + C2))
 *   ssim[b][t][c] = the mean of s over the plane's windows.
 * Frame PSNR = 10 log10(255^2 * 3 H W / sum_c sse) (inf for no error) and frame SSIM = the mean over c are the caller's, in fp64.
 * The entry leaves the last sum to the caller too: a workgroup handles one 16 x 16 tile of window positions of one plane, and
 * partials[B*T*3][tiles][2] int32 (plane = (b*T + t)*3 + c; tiles = gsdd_paired_metrics_tiles(H, W) = n(H) n(W) with n(v) = 1 for
 * v <= 26 and ceil((v - 10) / 16) above, GSDD_E_ARG for a size below 1; rows of tiles top to bottom) gets
 * per tile {the squared error of the pixels the tile owns -- every pixel has one owner, the sum over the tiles is sse --, the bits of
 * the fp32 sum of s over the tile's windows}.  Every word is written by exactly one workgroup: nothing has to be zeroed, there are no
 * atomics and no memset (safe to capture), and the bits are the same in every run and whatever else the batch holds.  The moments are
 * accumulated in fp64 (every product level x level x weight is exact there), so a window's s is good to about 1e-11 and a tile's sum
 * to its one rounding to fp32; identical operands give s = 1.0 and ssim = 1.0 exactly.  With want_ssim = 0 only the integers are
 * formed (the second word is written as 0.0f) and any H, W >= 1 is taken; with want_ssim = 1, H < 11 or W < 11 is GSDD_E_ARG, as are
 * a form other than 0 / 1, sizes below 1, a plane of 2^31 pixels or more, and 2^31 workgroups or more -- before any launch. */
int64_t gsdd_paired_metrics_tiles(int H, int W);
int gsdd_paired_metrics(const void* a, int form_a, const void* b, int form_b, int B, int T, int H, int W, int want_ssim,
                        int32_t* partials, void* stream);

/* ------------------------------------------------------------------ LPIPS (gsdd_amd/lpips.py; csrc/lpips.hip)
 * LPIPS v0.1 (Zhang et al. 2018, "The Unreasonable Effectiveness of Deep Features as a Perceptual Metric"), net = alex or vgg, per frame
 * pair of two clips in gsdd_paired_metrics' operand forms (form 0: float32 planar, a level by the uint8 rule; form 1: uint8 interleaved).
 *   1. input    x = level / 127.5 - 1, then (x - shift[c]) / scale[c] with shift = (-0.030, -0.088, -0.188), scale = (0.458, 0.448, 0.450).
 *               Only 3 x 256 values exist, so the rule IS the table
 *                 table[c * 256 + level] = (float)((level / 127.5 - 1.0 - shift[c]) / scale[c])     evaluated in fp64, rounded once,
 *               which the caller forms on the host and hands over.  The first convolution pads with ZERO IN THE SCALED SPACE (not with
 *               level 0, which maps to about -2.1).
 *   2. towers   torchvision's `features`: ReLU after every convolution, max pools in floor mode without padding.
 *                 alex  conv 3->64 k11 s4 p2 | pool 3 s2 | conv 64->192 k5 p2 | pool 3 s2 | conv 192->384 k3 p1 | conv 384->256 k3 p1 |
 *                       conv 256->256 k3 p1; taps: the five ReLU outputs, C = (64, 192, 384, 256, 256); frames of 31 x 31 and above
 *                 vgg   VGG-16's thirteen k3 p1 convolutions, pool 2 s2 behind the 2nd, 4th, 7th and 10th; taps: relu1_2, 2_2, 3_3, 4_3,
 *                       5_3, C = (64, 128, 256, 512, 512); frames of 16 x 16 and above
 *               (gsdd_gemm with bias + ReLU epilogue and gsdd_pool3d; the layer table is data in gsdd_amd/lpips.py).
 *   3. per tap k, over the P positions of the tap's map: a^ = a / (sqrt(sum_c a_c^2) + 1e-10), the same for b (eps OUTSIDE the root: an
 *               all-zero feature vector gives 0, not NaN), d_k = (1 / P) sum_p sum_c w_kc (a^_c - b^_c)^2 with the learned w_k >= 0
 *               (lin{k}.model.1.weight).  LPIPS = sum_k d_k: unscaled, >= 0, 0 for equal frames.
 *
 * gsdd_lpips_stem_rows: frames frame0 .. frame0 + n - 1 (frame = b T + t) of x -> out[n][H][W + 2 padw][4] floats, the first
 * convolution's operand with kw merged into the contraction (rows of 4 floats per pixel = the three table values and 0; the padw
 * columns in front of and behind a row are 0; the convolution's taps then run over kh alone, each a run of kw * 4 floats).  Every
 * float of out is written.  GSDD_E_ARG before the launch for a null pointer, a form other than 0 / 1, sizes below 1, padw outside
 * 0 .. 64, frames outside the clips, a float operand or table off 4-byte alignment, out off 16-byte alignment.
 *
 * gsdd_lpips_layer_distance: feat[2 n P][C] channels-last rows of one tap -- the n pred frames first, then the n target frames -- and
 * w[C] -> partials[n][slots] doubles, slots = gsdd_lpips_distance_slots(P, C) = ceil(P / (32 * 64 / G)) with G = min(64, the power
 * of two at or above C / 4) the lanes that share a position.  partials[i][s] is sum_c w_c (a^_c - b^_c)^2 summed over the positions
 * of slot s of frame pair i; d = (sum over s) / P is the caller's, in fp64.  Elements are read once as float4s and normalised by a
 * multiplication with 1 / (sqrt(sum) + 1e-10) in fp32; sums over positions are fp64.  Every word of partials is written by exactly one
 * workgroup: no atomics, nothing to zero (safe to capture), the same bits in every run and whatever else the batch holds; equal halves
 * give exactly 0.  GSDD_E_ARG before the launch for a null pointer, C not a multiple of 4 in 4 .. 512, n or P below 1, 2 n P of 2^31
 * or more, feat or w off 16-byte alignment, partials off 8-byte alignment. */
int gsdd_lpips_stem_rows(const void* x, int form, int B, int T, int H, int W, int64_t frame0, int64_t n, int padw, const float* table,
                         float* out, void* stream);
int64_t gsdd_lpips_distance_slots(int64_t P, int C);
int gsdd_lpips_layer_distance(const float* feat, const float* w, int64_t n, int64_t P, int C, double* partials, void* stream);

/* ------------------------------------------------------------------ hipGraph capture of a step
 * (the 100-iteration loop at diffusion_transformer.py:621-626 becomes 100 replays). */
int gsdd_graph_begin(void* stream);
int gsdd_graph_end(void* stream, void** graph_exec_out);
int gsdd_graph_launch(void* graph_exec, void* stream);
int gsdd_graph_destroy(void* graph_exec);

/* ------------------------------------------------------------------ clip preprocessing (next row)
 * replaces `preprocess` (src/datamodules/datasets/ucf101_dataset.py:105-140): uint8 frames video[N][T][H][W][3] ->
 * out[N][3][t_out][R][R] float32 = centre crop (h_start, w_start) of the bilinear resize (align_corners false) to th x tw of
 * (x/255 - ImageNet mean)/std; the first t_out frames of each clip (temporal crop, :116-118). */
int gsdd_preprocess_clip(const uint8_t* video, int N, int T, int H, int W, int t_out, int th, int tw, int h_start, int w_start,
                         int R, float* out, void* stream);

/* HIP-event timing on a given stream (bench.py measures the stream the kernels run on) */
int gsdd_event_create(void** ev);
int gsdd_event_record(void* ev, void* stream);
int gsdd_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms);   /* synchronises ev_stop */
int gsdd_event_destroy(void* ev);

#ifdef __cplusplus
}
#endif
#endif /* GSDD_H */
