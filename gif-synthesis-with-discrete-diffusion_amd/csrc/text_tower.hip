// The ends and the attention of the CLIP text tower (clip.model.CLIP.encode_text, called by the reference at
// src/models/text_models/clip_text_embedding.py:56-65): token + position embedding, causal multi-head self-attention over a
// context of at most 77 positions, and the gather of the end-of-text row.  The tower's linears, LayerNorms and QuickGELU are
// gsdd_gemm / gsdd_row_stats calls (gemm.hip); gif-synthesis-with-discrete-diffusion_amd/text.py strings them together.
//
// Attention: one workgroup per (batch element, head), one wave per 16-query tile (at most five).  The workgroup copies the
// head's Q (pre-scaled), K and V rows into LDS once, coalesced; rows behind S are written as zeros.  All products are 16x16
// tiles of v_mfma_f32_16x16x4_f32 (exact f32 multiply-add, the operand maps of axial_attention_mfma.hip):
//   A operand: lane (li = l & 15, g = l >> 4) gives A[li][k = g];  B operand: lane gives B[k = g][li];
//   result: lane holds D[4 g + r][li], r = 0..3.
// A score tile computed as K Q^T has the query on the lane and keys 4 g + r in registers, which is the A operand of the product
// with V when the contraction walks the keys of a tile in the order (r outer, g inner): the probabilities never leave registers.
// Wave qt computes key tiles 0 .. qt only -- a tile wholly above the diagonal is never touched -- and masks key > query in all of
// them (a no-op below the diagonal tile).  exp(-inf - m) is an exact 0 and the V rows behind S are zeros, so the tail of the
// last tile contributes exact zeros.
// LDS rows are D + 4 floats: the score operands read [16 rows][4 consecutive floats] (banks 4 li + g, all distinct) and the V
// operand reads [4 rows 4 apart][16 consecutive floats] (banks 16 g + li): neither conflicts, for D = 64, 32 and 16 alike.
#include "common.hpp"

namespace gsdd {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TEXT_MAX_S = 77;                    // CLIP's context length
constexpr int TEXT_TILES = (TEXT_MAX_S + 15) / 16;
constexpr int TEXT_ROWS = 16 * TEXT_TILES;

__device__ __forceinline__ float4 nan4() {
    const float n = __uint_as_float(0x7FC00000u);
    return make_float4(n, n, n, n);
}

// one thread per float4 of x[B*S][C]; an id outside the table reads nothing and leaves a NaN row (the host entry point rejects it
// beforehand when it is given the ids' host copy)
__global__ __launch_bounds__(256) void text_embed_kernel(const int64_t* __restrict__ ids, int64_t rows, int S, int ids_pitch, int C,
                                                         const float* __restrict__ tok_emb, int vocab,
                                                         const float* __restrict__ pos_emb, float* __restrict__ x) {
    const int c4n = C >> 2;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * c4n) return;
    const int64_t row = i / c4n;
    const int c = (int)(i - row * c4n) * 4;
    const int64_t b = row / S;
    const int s = (int)(row - b * S);
    const int64_t id = ids[b * ids_pitch + s];
    float4 v = nan4();
    if (id >= 0 && id < vocab) {
        const float4 e = *reinterpret_cast<const float4*>(tok_emb + id * C + c);
        const float4 p = *reinterpret_cast<const float4*>(pos_emb + (int64_t)s * C + c);
        v = make_float4(e.x + p.x, e.y + p.y, e.z + p.z, e.w + p.w);
    }
    *reinterpret_cast<float4*>(x + row * C + c) = v;
}

// one thread per float4 of out[B][C] = x[b*S + eot[b]][:]; an eot outside [0, S) reads nothing and leaves a NaN row
__global__ __launch_bounds__(256) void text_pool_kernel(const float* __restrict__ x, const int64_t* __restrict__ eot, int B, int S,
                                                        int C, float* __restrict__ out) {
    const int c4n = C >> 2;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * c4n) return;
    const int64_t b = i / c4n;
    const int c = (int)(i - b * c4n) * 4;
    const int64_t e = eot[b];
    float4 v = nan4();
    if (e >= 0 && e < S) v = *reinterpret_cast<const float4*>(x + (b * S + e) * C + c);
    *reinterpret_cast<float4*>(out + b * C + c) = v;
}

__device__ __forceinline__ float text_groups_max(float v) { v = fmaxf(v, __shfl_xor(v, 16)); return fmaxf(v, __shfl_xor(v, 32)); }
__device__ __forceinline__ float text_groups_sum(float v) { v += __shfl_xor(v, 16); return v + __shfl_xor(v, 32); }

// qkv rows [B*S][3C] = (q | k | v), head h at columns h*D of each third; out rows [B*S][C].  blockDim.x = 64 * ceil(S / 16).
template <int D>
__global__ __launch_bounds__(64 * TEXT_TILES) void text_attention_kernel(const float* __restrict__ qkv, int S, int C, int n_head,
                                                                         float scale, float* __restrict__ out) {
    constexpr int P = D + 4;
    __shared__ __attribute__((aligned(16))) float sq[TEXT_ROWS * P];
    __shared__ __attribute__((aligned(16))) float sk[TEXT_ROWS * P];
    __shared__ __attribute__((aligned(16))) float sv[TEXT_ROWS * P];
    const int b = blockIdx.x / n_head, h = blockIdx.x - b * n_head;
    const int nrow = 16 * (blockDim.x >> 6);                       // S rounded up to whole tiles, <= TEXT_ROWS
    const float* base = qkv + (int64_t)b * S * 3 * C + h * D;
    for (int i = threadIdx.x; i < nrow * (D / 4); i += blockDim.x) {
        const int r = i / (D / 4), c = 4 * (i - r * (D / 4));
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f), k = q, v = q;
        if (r < S) {
            const float* p = base + (int64_t)r * 3 * C + c;
            q = *reinterpret_cast<const float4*>(p);
            k = *reinterpret_cast<const float4*>(p + C);
            v = *reinterpret_cast<const float4*>(p + 2 * C);
            q = make_float4(q.x * scale, q.y * scale, q.z * scale, q.w * scale);      // q scaled before the product, as encode_text does
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
    // scores with the query on the lane: p[kt][r] = <q[query], k[16 kt + 4 g + r]>, -inf above the diagonal
    float p[TEXT_TILES][4];
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < TEXT_TILES; ++kt) {
        if (kt <= qt) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const float* kr = sk + (16 * kt + li) * P + g;
#pragma unroll
            for (int s = 0; s < D / 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[4 * s], q[s], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                p[kt][r] = (16 * kt + 4 * g + r <= query) ? acc[r] : -INFINITY;
                m = fmaxf(m, p[kt][r]);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) p[kt][r] = -INFINITY;
        }
    }
    m = text_groups_max(m);                                        // key 0 is visible to every query: m is finite
    float l = 0.f;
#pragma unroll
    for (int kt = 0; kt < TEXT_TILES; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            p[kt][r] = expf(p[kt][r] - m);
            l += p[kt][r];
        }
    l = text_groups_sum(l);
    // o[t][r'] = O[16 qt + 4 g + r'][16 t + li] = sum over (kt, r, g) of P[li][16 kt + 4 g + r] V[16 kt + 4 g + r][16 t + li]
    f32x4 o[D / 16];
#pragma unroll
    for (int t = 0; t < D / 16; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < TEXT_TILES; ++kt) {
        if (kt <= qt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pn = p[kt][r] / l;                         // (a true division, as torch.softmax: 20 per lane)
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

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace gsdd

using namespace gsdd;

extern "C" int gsdd_text_embed(const int64_t* ids, const int64_t* ids_host, int B, int S, int ids_pitch, int C, const float* tok_emb,
                               int vocab, const float* pos_emb, int n_pos, float* x, void* stream) {
    GSDD_CHECK_ARG(ids && tok_emb && pos_emb && x, "null pointer");
    GSDD_CHECK_ARG(B > 0 && S >= 1 && S <= TEXT_MAX_S && S <= n_pos && ids_pitch >= S && vocab > 0, "bad sizes (1 <= S <= 77, S <= n_pos, ids_pitch >= S)");
    GSDD_CHECK_ARG(C > 0 && C % 4 == 0, "C must be a multiple of 4");
    GSDD_CHECK_ARG(aligned16(tok_emb) && aligned16(pos_emb) && aligned16(x), "tables and output must be 16-byte aligned");
    if (ids_host != nullptr) {
        for (int b = 0; b < B; ++b)
            for (int s = 0; s < S; ++s) {
                const int64_t id = ids_host[(int64_t)b * ids_pitch + s];
                if (id < 0 || id >= vocab) {
                    set_error(std::string(__func__) + ": ids[" + std::to_string(b) + "][" + std::to_string(s) + "] = " + std::to_string(id) +
                              " is outside the vocabulary of " + std::to_string(vocab));
                    return GSDD_E_ARG;
                }
            }
    }
    const int64_t rows = (int64_t)B * S, n = rows * (C / 4);
    GSDD_CHECK_ARG((n + 255) / 256 < (1ll << 31), "too many elements");
    hipLaunchKernelGGL(text_embed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ids, rows, S, ids_pitch,
                       C, tok_emb, vocab, pos_emb, x);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}

extern "C" int gsdd_text_attention(const float* qkv, int B, int S, int C, int n_head, float scale, float* out, void* stream) {
    GSDD_CHECK_ARG(qkv && out, "null pointer");
    GSDD_CHECK_ARG(B > 0 && S >= 1 && S <= TEXT_MAX_S, "1 <= S <= 77");
    GSDD_CHECK_ARG(C > 0 && n_head > 0 && C % n_head == 0 && (C / n_head == 64 || C / n_head == 32 || C / n_head == 16),
                   "head dimension must be 64, 32 or 16");
    GSDD_CHECK_ARG((int64_t)B * n_head < (1ll << 31), "too many (batch, head) pairs");
    GSDD_CHECK_ARG(aligned16(qkv), "qkv must be 16-byte aligned");
    GSDD_CHECK_ARG(scale == scale && scale > 0.f && scale < INFINITY, "scale must be finite and positive");
    const dim3 grid((unsigned)(B * n_head)), block(64 * ((S + 15) / 16));
    if (C / n_head == 64) hipLaunchKernelGGL(text_attention_kernel<64>, grid, block, 0, (hipStream_t)stream, qkv, S, C, n_head, scale, out);
    else if (C / n_head == 32) hipLaunchKernelGGL(text_attention_kernel<32>, grid, block, 0, (hipStream_t)stream, qkv, S, C, n_head, scale, out);
    else hipLaunchKernelGGL(text_attention_kernel<16>, grid, block, 0, (hipStream_t)stream, qkv, S, C, n_head, scale, out);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}

extern "C" int gsdd_text_pool(const float* x, const int64_t* eot, const int64_t* eot_host, int B, int S, int C, float* out, void* stream) {
    GSDD_CHECK_ARG(x && eot && out, "null pointer");
    GSDD_CHECK_ARG(B > 0 && S >= 1 && S <= TEXT_MAX_S, "1 <= S <= 77");
    GSDD_CHECK_ARG(C > 0 && C % 4 == 0, "C must be a multiple of 4");
    GSDD_CHECK_ARG(aligned16(x) && aligned16(out), "rows must be 16-byte aligned");
    if (eot_host != nullptr) {
        for (int b = 0; b < B; ++b)
            if (eot_host[b] < 0 || eot_host[b] >= S) {
                set_error(std::string(__func__) + ": eot[" + std::to_string(b) + "] = " + std::to_string(eot_host[b]) + " is outside [0, " +
                          std::to_string(S) + ")");
                return GSDD_E_ARG;
            }
    }
    const int64_t n = (int64_t)B * (C / 4);
    hipLaunchKernelGGL(text_pool_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, eot, B, S, C, out);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}
