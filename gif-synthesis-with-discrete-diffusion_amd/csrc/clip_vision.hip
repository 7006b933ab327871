// The pieces of the CLIP image tower (clip.model.VisionTransformer / transformers.CLIPVisionModelWithProjection) that are not a
// gsdd_gemm / gsdd_row_stats / gsdd_ln_apply / gsdd_text_pool call: frames -> patch rows, class token + position embedding, and the
// NON-causal multi-head self-attention over at most 77 positions.  gif-synthesis-with-discrete-diffusion_amd/vision.py strings the
// tower together; the evaluator scores sampled clips against their captions with it (CLIPSIM).
//
// Frame patches.  One thread per resized pixel (frame, channel, y, x) of the R x R image.  The source pixels are the decoder's
// ImageNet-normalised floats; each of the 4 x 4 taps is de-normalised and quantised to its uint8 level exactly as the evaluator's
// _prepare does (x * std + mean, x 255, truncated, clamped), kept as level / 255.  The resize is TORCH's bicubic
// (F.interpolate(mode="bicubic", align_corners=False, antialias=False)): Keys' kernel with a = -0.75, source coordinate
// (o + 0.5) H / R - 0.5, border indices clamped, rows first and then the column -- NOT PIL's (a = -0.5, fixed-point weights,
// antialiasing when shrinking), which the `clip` package's preprocessing uses; parity with that is not claimed.  The source
// coordinate is the rational ((2 o + 1) H - R) / (2 R): its floor and its fraction are taken in integers, so the weights carry one
// rounding of t and not the rounding of a coordinate near H (torch forms the coordinate in fp32).  At H == R every fraction is 0,
// the weights are exactly (0, 1, 0, 0) and the result is the quantised frame.
//
// Attention.  text_tower.hip's layout: one workgroup per (row, head), one wave per 16-query tile (at most five), Q (pre-scaled), K
// and V of the head in LDS at a pitch of D + 4 floats (rows behind S written as zeros), every product a 16x16 tile of
// v_mfma_f32_16x16x4_f32 (exact f32; operand maps: A lane (li = l & 15, g = l >> 4) gives A[li][k = g], B gives B[k = g][li], the
// result D[4 g + r][li], r = 0..3).  Scores are computed as K Q^T -- query on the lane, keys 4 g + r in registers -- which is the
// A operand of the product with V, so the probabilities never leave registers.  What differs from the causal kernel: EVERY wave
// walks ALL ceil(S / 16) key tiles, and nothing causal hides the zero-filled tail of the last one (a zero K row scores 0, which
// is a probability of exp(-m) and not of 0), so keys at positions >= S are set to -inf BEFORE the row maximum and the sum.
// exp(-inf - m) is an exact 0 and the V rows behind S are zeros: the tail contributes exact zeros.  Query rows at positions >= S
// of the last wave's tile compute on zero Q rows (finite throughout) and are not stored.
#include "common.hpp"

namespace gsdd {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int CLIPV_MAX_S = 77;                   // the attention kernel's LDS images hold 80 rows
constexpr int CLIPV_TILES = (CLIPV_MAX_S + 15) / 16;
constexpr int CLIPV_ROWS = 16 * CLIPV_TILES;

struct ClipNorm { float im_mean[3], im_std[3], clip_mean[3], clip_std[3]; };

// torch's cubic convolution coefficients (UpSample.h get_cubic_upsample_coefficients, A = -0.75) for taps i0 - 1 .. i0 + 2
__device__ __forceinline__ void cubic_weights(float t, float w[4]) {
    const float A = -0.75f;
    const float x0 = t + 1.f, x1 = t, x2 = 1.f - t, x3 = 2.f - t;
    w[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
    w[1] = ((A + 2.f) * x1 - (A + 3.f)) * x1 * x1 + 1.f;
    w[2] = ((A + 2.f) * x2 - (A + 3.f)) * x2 * x2 + 1.f;
    w[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
}

// floor and fraction of ((2 o + 1) H - R) / (2 R), o in [0, R), H <= R: the numerator is >= H - R > -2 R, so the floor is >= -1
__device__ __forceinline__ void source_coord(int o, int H, int R, int& i0, float& t) {
    const int num = (2 * o + 1) * H - R, den = 2 * R;
    i0 = num >= 0 ? num / den : -1;
    t = (float)(num - i0 * den) / (float)den;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// clips [B][3][T][H][H] -> out rows [(b T + t) G^2 + gy G + gx][c P P + py P + px], G = R / P
__global__ __launch_bounds__(256) void clip_frame_patches_kernel(const float* __restrict__ clips, int64_t frames, int T, int H, int R, int P,
                                                                 ClipNorm nm, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t plane = (int64_t)R * R;
    if (i >= frames * 3 * plane) return;
    const int64_t fc = i / plane;
    const int rem = (int)(i - fc * plane);
    const int oy = rem / R, ox = rem - oy * R;
    const int64_t n = fc / 3;
    const int c = (int)(fc - n * 3);
    const int64_t b = n / T;
    const int tt = (int)(n - b * T);
    const float* src = clips + ((b * 3 + c) * T + tt) * (int64_t)H * H;
    int y0, x0;
    float ty, tx, wy[4], wx[4];
    source_coord(oy, H, R, y0, ty);
    source_coord(ox, H, R, x0, tx);
    cubic_weights(ty, wy);
    cubic_weights(tx, wx);
    const float mean = nm.im_mean[c], std = nm.im_std[c];
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float* row = src + (int64_t)clampi(y0 - 1 + k, 0, H - 1) * H;
        float r = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float v = row[clampi(x0 - 1 + j, 0, H - 1)] * std + mean;
            const float level = fminf(fmaxf(truncf(v * 255.f), 0.f), 255.f);      // (fmaxf drops a NaN: level 0)
            r += wx[j] * (level / 255.f);
        }
        acc += wy[k] * r;
    }
    acc = fminf(fmaxf(acc, 0.f), 1.f);
    const int G = R / P;
    const int gy = oy / P, py = oy - gy * P, gx = ox / P, px = ox - gx * P;
    const int64_t orow = (n * G + gy) * G + gx;
    out[orow * (3 * P * P) + (c * P + py) * P + px] = (acc - nm.clip_mean[c]) / nm.clip_std[c];
}

// one thread per float4 of x[N*S][C]: row s = 0 is class_emb + pos[0], row 1 + p is patches[n (S - 1) + p] + pos[1 + p]
__global__ __launch_bounds__(256) void clip_vision_embed_kernel(const float* __restrict__ patches, const float* __restrict__ class_emb,
                                                                const float* __restrict__ pos, int64_t rows, int S, int C,
                                                                float* __restrict__ x) {
    const int c4n = C >> 2;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * c4n) return;
    const int64_t row = i / c4n;
    const int c = (int)(i - row * c4n) * 4;
    const int64_t n = row / S;
    const int s = (int)(row - n * S);
    const float* e = s == 0 ? class_emb + c : patches + (n * (S - 1) + (s - 1)) * C + c;
    const float4 a = *reinterpret_cast<const float4*>(e);
    const float4 p = *reinterpret_cast<const float4*>(pos + (int64_t)s * C + c);
    *reinterpret_cast<float4*>(x + row * C + c) = make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
}

__device__ __forceinline__ float clipv_groups_max(float v) { v = fmaxf(v, __shfl_xor(v, 16)); return fmaxf(v, __shfl_xor(v, 32)); }
__device__ __forceinline__ float clipv_groups_sum(float v) { v += __shfl_xor(v, 16); return v + __shfl_xor(v, 32); }

// qkv rows [B*S][3C] = (q | k | v), head h at columns h*D of each third; out rows [B*S][C].  blockDim.x = 64 * ceil(S / 16).
template <int D>
__global__ __launch_bounds__(64 * CLIPV_TILES) void clip_attention_kernel(const float* __restrict__ qkv, int S, int C, int n_head,
                                                                          float scale, float* __restrict__ out) {
    constexpr int P = D + 4;
    __shared__ __attribute__((aligned(16))) float sq[CLIPV_ROWS * P];
    __shared__ __attribute__((aligned(16))) float sk[CLIPV_ROWS * P];
    __shared__ __attribute__((aligned(16))) float sv[CLIPV_ROWS * P];
    const int b = blockIdx.x / n_head, h = blockIdx.x - b * n_head;
    const int nt = __builtin_amdgcn_readfirstlane((int)(blockDim.x >> 6));      // key (and query) tiles, <= CLIPV_TILES
    const int nrow = 16 * nt;                                      // S rounded up to whole tiles, <= CLIPV_ROWS
    const float* base = qkv + (int64_t)b * S * 3 * C + h * D;
    for (int i = threadIdx.x; i < nrow * (D / 4); i += blockDim.x) {
        const int r = i / (D / 4), c = 4 * (i - r * (D / 4));
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f), k = q, v = q;
        if (r < S) {
            const float* p = base + (int64_t)r * 3 * C + c;
            q = *reinterpret_cast<const float4*>(p);
            k = *reinterpret_cast<const float4*>(p + C);
            v = *reinterpret_cast<const float4*>(p + 2 * C);
            q = make_float4(q.x * scale, q.y * scale, q.z * scale, q.w * scale);      // q scaled before the product, as the tower does
        }
        *reinterpret_cast<float4*>(sq + r * P + c) = q;
        *reinterpret_cast<float4*>(sk + r * P + c) = k;
        *reinterpret_cast<float4*>(sv + r * P + c) = v;
    }
    __syncthreads();

    const int qt = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
    const int query = 16 * qt + li;
    float q[D / 4];
#pragma unroll
    for (int s = 0; s < D / 4; ++s) q[s] = sq[query * P + 4 * s + g];
    // scores with the query on the lane: p[kt][r] = <q[query], k[16 kt + 4 g + r]>, -inf for a key behind S
    float p[CLIPV_TILES][4];
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < CLIPV_TILES; ++kt) {
        if (kt < nt) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const float* kr = sk + (16 * kt + li) * P + g;
#pragma unroll
            for (int s = 0; s < D / 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[4 * s], q[s], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                p[kt][r] = (16 * kt + 4 * g + r < S) ? acc[r] : -INFINITY;
                m = fmaxf(m, p[kt][r]);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) p[kt][r] = -INFINITY;
        }
    }
    m = clipv_groups_max(m);                                       // key 0 is in front of S for every query: m is finite
    float l = 0.f;
#pragma unroll
    for (int kt = 0; kt < CLIPV_TILES; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            p[kt][r] = expf(p[kt][r] - m);
            l += p[kt][r];
        }
    l = clipv_groups_sum(l);
    // o[t][r'] = O[16 qt + 4 g + r'][16 t + li] = sum over (kt, r, g) of P[li][16 kt + 4 g + r] V[16 kt + 4 g + r][16 t + li]
    f32x4 o[D / 16];
#pragma unroll
    for (int t = 0; t < D / 16; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < CLIPV_TILES; ++kt) {
        if (kt < nt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pn = p[kt][r] / l;                         // (a true division, as torch.softmax)
                const float* vr = sv + (16 * kt + 4 * g + r) * P + li;
#pragma unroll
                for (int t = 0; t < D / 16; ++t) o[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(pn, vr[16 * t], o[t], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 16 * qt + 4 * g + r;
        if (row < S) {
            float* dst = out + ((int64_t)b * S + row) * C + h * D + li;
#pragma unroll
            for (int t = 0; t < D / 16; ++t) dst[16 * t] = o[t][r];
        }
    }
}

static inline bool clipv_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace gsdd

using namespace gsdd;

extern "C" int gsdd_clip_frame_patches(const float* clips, int B, int T, int H, int W, int R, int P, float* out, void* stream) {
    GSDD_CHECK_ARG(clips && out, "null pointer");
    GSDD_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && R > 0 && P > 0, "bad sizes");
    GSDD_CHECK_ARG(H == W, "frames must be square (a non-square frame needs a crop this entry point does not do)");
    GSDD_CHECK_ARG(H <= R && R <= 4096, "H <= R <= 4096: the resize only enlarges (shrinking needs antialiasing)");
    GSDD_CHECK_ARG(R % P == 0, "the resolution must be a multiple of the patch size");
    const int64_t frames = (int64_t)B * T;
    GSDD_CHECK_ARG(frames < (1ll << 31), "too many frames");
    const int64_t n = frames * 3 * R * R;                                          // (frames < 2^31, 3 R R < 2^26: no overflow)
    GSDD_CHECK_ARG((n + 255) / 256 < (1ll << 31), "too many elements");
    const ClipNorm nm = {{0.485f, 0.456f, 0.406f}, {0.229f, 0.224f, 0.225f}, {0.48145466f, 0.4578275f, 0.40821073f},
                         {0.26862954f, 0.26130258f, 0.27577711f}};
    hipLaunchKernelGGL(clip_frame_patches_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, clips, frames, T, H,
                       R, P, nm, out);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}

extern "C" int gsdd_clip_vision_embed(const float* patches, const float* class_emb, const float* pos, int N, int S, int C, float* x,
                                      void* stream) {
    GSDD_CHECK_ARG(patches && class_emb && pos && x, "null pointer");
    GSDD_CHECK_ARG(N > 0 && S >= 1 && S <= CLIPV_MAX_S, "1 <= S <= 77 (S = patches per frame + 1)");
    GSDD_CHECK_ARG(C > 0 && C % 4 == 0, "C must be a multiple of 4");
    GSDD_CHECK_ARG(clipv_aligned16(patches) && clipv_aligned16(class_emb) && clipv_aligned16(pos) && clipv_aligned16(x),
                   "rows must be 16-byte aligned");
    const int64_t rows = (int64_t)N * S;
    GSDD_CHECK_ARG(rows < (1ll << 31), "too many rows");
    const int64_t n = rows * (C / 4);
    GSDD_CHECK_ARG((n + 255) / 256 < (1ll << 31), "too many elements");
    hipLaunchKernelGGL(clip_vision_embed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, patches, class_emb,
                       pos, rows, S, C, x);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}

extern "C" int gsdd_clip_attention(const float* qkv, int B, int S, int C, int n_head, float scale, float* out, void* stream) {
    GSDD_CHECK_ARG(qkv && out, "null pointer");
    GSDD_CHECK_ARG(B > 0 && S >= 1 && S <= CLIPV_MAX_S, "1 <= S <= 77");
    GSDD_CHECK_ARG(C > 0 && n_head > 0 && C % n_head == 0 && (C / n_head == 64 || C / n_head == 32 || C / n_head == 16),
                   "head dimension must be 64, 32 or 16");
    GSDD_CHECK_ARG((int64_t)B * n_head < (1ll << 31), "too many (row, head) pairs");
    GSDD_CHECK_ARG(clipv_aligned16(qkv), "qkv must be 16-byte aligned");
    GSDD_CHECK_ARG(scale == scale && scale > 0.f && scale < INFINITY, "scale must be finite and positive");
    const dim3 grid((unsigned)(B * n_head)), block(64 * ((S + 15) / 16));
    if (C / n_head == 64) hipLaunchKernelGGL(clip_attention_kernel<64>, grid, block, 0, (hipStream_t)stream, qkv, S, C, n_head, scale, out);
    else if (C / n_head == 32) hipLaunchKernelGGL(clip_attention_kernel<32>, grid, block, 0, (hipStream_t)stream, qkv, S, C, n_head, scale, out);
    else hipLaunchKernelGGL(clip_attention_kernel<16>, grid, block, 0, (hipStream_t)stream, qkv, S, C, n_head, scale, out);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}
