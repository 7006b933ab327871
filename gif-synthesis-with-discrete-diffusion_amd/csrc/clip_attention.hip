// Multi-head self-attention over a sequence of at most 77 positions, for both CLIP towers: causal for the text tower
// (gsdd_text_attention, the nn.MultiheadAttention of clip.model.CLIP.encode_text under build_attention_mask) and with every query
// seeing every key for the image tower (gsdd_clip_attention, clip.model.VisionTransformer).  One kernel template; CAUSAL changes which
// key tiles a wave walks and which keys it masks, nothing else (the tile count is read the way each form needs it for that walk).
//
// One workgroup per (batch row, head), one wave per 16-query tile (at most five).  The workgroup copies the head's Q (pre-scaled), K
// and V rows into LDS once, coalesced; rows behind S are written as zeros.  All products are 16x16 tiles of v_mfma_f32_16x16x4_f32
// (exact f32 multiply-add, the operand maps of axial_attention_mfma.hip):
//   A operand: lane (li = l & 15, g = l >> 4) gives A[li][k = g];  B operand: lane gives B[k = g][li];
//   result: lane holds D[4 g + r][li], r = 0..3.
// A score tile computed as K Q^T has the query on the lane and keys 4 g + r in registers, which is the A operand of the product
// with V when the contraction walks the keys of a tile in the order (r outer, g inner): the probabilities never leave registers.
// Causal: wave qt computes key tiles 0 .. qt only -- a tile wholly above the diagonal is never touched -- and masks key > query in
// all of them (a no-op below the diagonal tile).  That needs no mask of the tail: a key behind S is behind every stored query, so it
// is above the diagonal already.
// Non-causal: EVERY wave walks ALL ceil(S / 16) key tiles, and nothing hides the zero-filled tail of the last one (a zero K row
// scores 0, which is a probability of exp(-m) and not of 0), so keys at positions >= S are set to -inf BEFORE the row maximum and
// the sum.
// Either way exp(-inf - m) is an exact 0 and the V rows behind S are zeros: the tail of the last tile contributes exact zeros.
// Query rows at positions >= S of the last wave's tile compute on zero Q rows (finite throughout) and are not stored.
// LDS rows are D + 4 floats: the score operands read [16 rows][4 consecutive floats] (banks 4 li + g, all distinct) and the V
// operand reads [4 rows 4 apart][16 consecutive floats] (banks 16 g + li): neither conflicts, for D = 64, 32 and 16 alike.
#include "common.hpp"

namespace gsdd {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int ATT_MAX_S = 77;                     // CLIP's context length; ViT-B/32 at 224 has 50 positions
constexpr int ATT_TILES = (ATT_MAX_S + 15) / 16;
constexpr int ATT_ROWS = 16 * ATT_TILES;          // the LDS images hold 80 rows

__device__ __forceinline__ float groups_max(float v) { v = fmaxf(v, __shfl_xor(v, 16)); return fmaxf(v, __shfl_xor(v, 32)); }
__device__ __forceinline__ float groups_sum(float v) { v += __shfl_xor(v, 16); return v + __shfl_xor(v, 32); }

// qkv rows [B*S][3C] = (q | k | v), head h at columns h*D of each third; out rows [B*S][C].  blockDim.x = 64 * ceil(S / 16).
template <int D, bool CAUSAL>
__global__ __launch_bounds__(64 * ATT_TILES) void clip_attention_kernel(const float* __restrict__ qkv, int S, int C, int n_head,
                                                                        float scale, float* __restrict__ out) {
    constexpr int P = D + 4;
    __shared__ __attribute__((aligned(16))) float sq[ATT_ROWS * P];
    __shared__ __attribute__((aligned(16))) float sk[ATT_ROWS * P];
    __shared__ __attribute__((aligned(16))) float sv[ATT_ROWS * P];
    const int b = blockIdx.x / n_head, h = blockIdx.x - b * n_head;
    // key (and query) tiles, <= ATT_TILES; the non-causal walk is bounded by it, so there it is made wave-uniform for the compiler
    const int nt = CAUSAL ? (int)(blockDim.x >> 6) : __builtin_amdgcn_readfirstlane((int)(blockDim.x >> 6));
    const int nrow = 16 * nt;                                      // S rounded up to whole tiles, <= ATT_ROWS
    const float* base = qkv + (int64_t)b * S * 3 * C + h * D;
    for (int i = threadIdx.x; i < nrow * (D / 4); i += blockDim.x) {
        const int r = i / (D / 4), c = 4 * (i - r * (D / 4));
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f), k = q, v = q;
        if (r < S) {
            const float* p = base + (int64_t)r * 3 * C + c;
            q = *reinterpret_cast<const float4*>(p);
            k = *reinterpret_cast<const float4*>(p + C);
            v = *reinterpret_cast<const float4*>(p + 2 * C);
            q = make_float4(q.x * scale, q.y * scale, q.z * scale, q.w * scale);      // q scaled before the product, as both towers do
        }
        *reinterpret_cast<float4*>(sq + r * P + c) = q;
        *reinterpret_cast<float4*>(sk + r * P + c) = k;
        *reinterpret_cast<float4*>(sv + r * P + c) = v;
    }
    __syncthreads();

    const int qt = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
    const int query = 16 * qt + li;
    // the last key tile this wave walks: its own (causal), or the last of the sequence
    const int last = CAUSAL ? qt : nt - 1;
    float q[D / 4];
#pragma unroll
    for (int s = 0; s < D / 4; ++s) q[s] = sq[query * P + 4 * s + g];
    // scores with the query on the lane: p[kt][r] = <q[query], k[16 kt + 4 g + r]>, -inf for a key the query does not see
    float p[ATT_TILES][4];
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < ATT_TILES; ++kt) {
        if (kt <= last) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const float* kr = sk + (16 * kt + li) * P + g;
#pragma unroll
            for (int s = 0; s < D / 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[4 * s], q[s], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = 16 * kt + 4 * g + r;
                p[kt][r] = (CAUSAL ? key <= query : key < S) ? acc[r] : -INFINITY;
                m = fmaxf(m, p[kt][r]);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) p[kt][r] = -INFINITY;
        }
    }
    m = groups_max(m);                                             // key 0 is visible to every query: m is finite
    float l = 0.f;
#pragma unroll
    for (int kt = 0; kt < ATT_TILES; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            p[kt][r] = expf(p[kt][r] - m);
            l += p[kt][r];
        }
    l = groups_sum(l);
    // o[t][r'] = O[16 qt + 4 g + r'][16 t + li] = sum over (kt, r, g) of P[li][16 kt + 4 g + r] V[16 kt + 4 g + r][16 t + li]
    f32x4 o[D / 16];
#pragma unroll
    for (int t = 0; t < D / 16; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < ATT_TILES; ++kt) {
        if (kt <= last) {
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

// the checks and the launch of both entry points; `fn` is the name of the one that was called, which its error texts begin with
template <bool CAUSAL>
static int attention_launch(const char* fn, const float* qkv, int B, int S, int C, int n_head, float scale, float* out, void* stream) {
    GSDD_CHECK_ARG_AS(fn, qkv && out, "null pointer");
    GSDD_CHECK_ARG_AS(fn, B > 0 && S >= 1 && S <= ATT_MAX_S, "1 <= S <= 77");
    GSDD_CHECK_ARG_AS(fn, C > 0 && n_head > 0 && C % n_head == 0 && (C / n_head == 64 || C / n_head == 32 || C / n_head == 16),
                      "head dimension must be 64, 32 or 16");
    GSDD_CHECK_ARG_AS(fn, (int64_t)B * n_head < (1ll << 31), CAUSAL ? "too many (batch, head) pairs" : "too many (row, head) pairs");
    GSDD_CHECK_ARG_AS(fn, aligned16(qkv), "qkv must be 16-byte aligned");
    GSDD_CHECK_ARG_AS(fn, scale == scale && scale > 0.f && scale < INFINITY, "scale must be finite and positive");
    const dim3 grid((unsigned)(B * n_head)), block(64 * ((S + 15) / 16));
    const int d = C / n_head;
    auto* kernel = d == 64 ? clip_attention_kernel<64, CAUSAL> : d == 32 ? clip_attention_kernel<32, CAUSAL> : clip_attention_kernel<16, CAUSAL>;
    hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, qkv, S, C, n_head, scale, out);
    GSDD_CHECK_HIP_AS(fn, hipGetLastError());
    return GSDD_OK;
}

}  // namespace gsdd

using namespace gsdd;

extern "C" int gsdd_text_attention(const float* qkv, int B, int S, int C, int n_head, float scale, float* out, void* stream) {
    return attention_launch<true>(__func__, qkv, B, S, C, n_head, scale, out, stream);
}

extern "C" int gsdd_clip_attention(const float* qkv, int B, int S, int C, int n_head, float scale, float* out, void* stream) {
    return attention_launch<false>(__func__, qkv, B, S, C, n_head, scale, out, stream);
}
