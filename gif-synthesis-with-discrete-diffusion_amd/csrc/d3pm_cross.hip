// Cross-attention of the denoiser over Te condition tokens, training versions: forward with log-sum-exp and the backward.
// Head dim 4, q head-major [H][M][4] (M = B L), kc / vc rows [B Te][H 4], out / o / dO rows [M][H 4], scores q.k / 2
// (transformer_utils.py:95-113).  Everything is plain f32 on the vector ALU: Te <= 77 keys per row make the products tiny (23 M
// scores at bs 16, L = 4096, Te = 22) and the kernels are bound by the rows they move, not by arithmetic.
//
// Backward.  P is formed from the saved lse (no row reduction), delta = dO . o per (row, head).
//   cross_bwd_dq_kernel     one lane per (row, head): dq (head-major) and delta (workspace), a loop over the Te keys of the row's
//                           batch element.  The batch element is found per lane (b = m / L): a block's rows may straddle several.
//   cross_bwd_dkv_kernel    dkc / dvc are sums over the L rows of a batch element.  The grid is built per batch element: block
//                           (chunk c of CR_ROWS rows of batch element b, group of CR_PAIRS (head, key) pairs), one lane per (head, key)
//                           pair, which walks the chunk's rows in ascending order and keeps its 8 sums in registers -> one partial
//                           per (b, chunk, head, key) in the caller's workspace.
//   cross_bwd_reduce_kernel one lane per output element adds the partials of its batch element in ascending chunk order.
// No atomics, and no sum whose order depends on the grid's scheduling: the same inputs give the same bits on every run, and a batch
// element's results do not depend on which other elements share the launch.
// Workspace (gsdd_d3pm_cross_attention_bwd_workspace_bytes): delta f32 [H][M], padded to 256 B | partials f32 [B][chunks][H][Te][8]
// ({dk x 4 (before the 1/2), dv x 4}).
//
// Condition lengths (the _len entry points): cond_len, int32 [B], is a kernel argument, NULL in the entry points without lengths.  With
// it, batch element b attends to its keys 0 .. len[b] - 1 only (a prefix; len[b] clamped into [1, Te] on the device), keys behind it
// are never read, and the dK / dV lane of such a key skips its rows and writes a zero partial, so that the reduce kernel, which knows
// nothing of lengths, writes exact zeros into those dkc / dvc rows.  The loops run the same arithmetic in the same order over len[b]
// keys as over Te: without lengths, and with every length equal to Te, the bits are the ones they always were.
#include "common.hpp"

namespace gsdd {

constexpr int CR_ROWS = 64;       // query rows per dK / dV partial
constexpr int CR_PAIRS = 128;     // (head, key) pairs per block of the dK / dV kernel
constexpr float CR_C = 0.5f * 1.4426950408889634f;     // 1/2 (the score scale) times log2(e): scores in the log2 domain

__host__ __device__ __forceinline__ int64_t cross_delta_bytes(int64_t M, int H) { return (M * H * 4 + 255) & ~(int64_t)255; }
__host__ __device__ __forceinline__ int cross_chunks(int L) { return (L + CR_ROWS - 1) / CR_ROWS; }
// keys of batch element b: its length clamped into [1, Te] (never an empty softmax, never a row outside kc / vc); no lengths: all Te
__device__ __forceinline__ int cross_keys(const int32_t* cond_len, int b, int Te) {
    return cond_len != nullptr ? min(max(cond_len[b], 1), Te) : Te;
}

// forward: one lane per (row, head), online softmax over the keys (one pass over kc / vc)
__global__ __launch_bounds__(256) void cross_train_fwd_kernel(const float* q, const float* kc, const float* vc, const int32_t* cond_len,
                                                              int B, int L, int Te, int H, float* out, float* lse) {
    const int64_t M = (int64_t)B * L;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * H) return;
    const int h = (int)(i / M);
    const int64_t m = i - (int64_t)h * M;
    const int b = (int)(m / L);
    float4 qv = *reinterpret_cast<const float4*>(q + i * 4);
    qv.x *= CR_C; qv.y *= CR_C; qv.z *= CR_C; qv.w *= CR_C;
    const float* kp = kc + (int64_t)b * Te * (H * 4) + h * 4;
    const float* vp = vc + (int64_t)b * Te * (H * 4) + h * 4;
    const int ne = cross_keys(cond_len, b, Te);
    float mx = -INFINITY, l = 0.f, o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f;
    for (int e = 0; e < ne; ++e) {
        const float4 kk = *reinterpret_cast<const float4*>(kp + (int64_t)e * (H * 4));
        const float4 vv = *reinterpret_cast<const float4*>(vp + (int64_t)e * (H * 4));
        const float s = fmaf(qv.x, kk.x, fmaf(qv.y, kk.y, fmaf(qv.z, kk.z, qv.w * kk.w)));
        if (s > mx) {
            const float a = __builtin_amdgcn_exp2f(mx - s);
            l *= a; o0 *= a; o1 *= a; o2 *= a; o3 *= a;
            mx = s;
        }
        const float p = __builtin_amdgcn_exp2f(s - mx);
        l += p;
        o0 = fmaf(p, vv.x, o0); o1 = fmaf(p, vv.y, o1); o2 = fmaf(p, vv.z, o2); o3 = fmaf(p, vv.w, o3);
    }
    const float inv = 1.f / l;
    *reinterpret_cast<float4*>(out + m * (H * 4) + h * 4) = make_float4(o0 * inv, o1 * inv, o2 * inv, o3 * inv);
    lse[i] = mx + log2f(l);       // log2 domain, as gsdd_d3pm_attention_train keeps it
}

// dQ (head-major) and delta = dO . o: one lane per (row, head)
__global__ __launch_bounds__(256) void cross_bwd_dq_kernel(const float* q, const float* kc, const float* vc, const float* o,
                                                           const float* dO, const float* lse, const int32_t* cond_len, int B, int L,
                                                           int Te, int H, float* dq, float* delta) {
    const int64_t M = (int64_t)B * L;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * H) return;
    const int h = (int)(i / M);
    const int64_t m = i - (int64_t)h * M;
    const int b = (int)(m / L);
    float4 qv = *reinterpret_cast<const float4*>(q + i * 4);
    qv.x *= CR_C; qv.y *= CR_C; qv.z *= CR_C; qv.w *= CR_C;
    const float4 g = *reinterpret_cast<const float4*>(dO + m * (H * 4) + h * 4);
    const float4 ov = *reinterpret_cast<const float4*>(o + m * (H * 4) + h * 4);
    const float Dq = (g.x * ov.x + g.y * ov.y) + (g.z * ov.z + g.w * ov.w);
    const float ls = lse[i];
    const float* kp = kc + (int64_t)b * Te * (H * 4) + h * 4;
    const float* vp = vc + (int64_t)b * Te * (H * 4) + h * 4;
    const int ne = cross_keys(cond_len, b, Te);
    float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
    for (int e = 0; e < ne; ++e) {
        const float4 kk = *reinterpret_cast<const float4*>(kp + (int64_t)e * (H * 4));
        const float4 vv = *reinterpret_cast<const float4*>(vp + (int64_t)e * (H * 4));
        const float s = fmaf(qv.x, kk.x, fmaf(qv.y, kk.y, fmaf(qv.z, kk.z, qv.w * kk.w)));
        const float p = __builtin_amdgcn_exp2f(s - ls);
        const float dp = fmaf(g.x, vv.x, fmaf(g.y, vv.y, fmaf(g.z, vv.z, g.w * vv.w)));
        const float ds = p * (dp - Dq);
        d0 = fmaf(ds, kk.x, d0); d1 = fmaf(ds, kk.y, d1); d2 = fmaf(ds, kk.z, d2); d3 = fmaf(ds, kk.w, d3);
    }
    *reinterpret_cast<float4*>(dq + i * 4) = make_float4(0.5f * d0, 0.5f * d1, 0.5f * d2, 0.5f * d3);
    delta[i] = Dq;
}

// dK / dV partials of one chunk of rows of one batch element: one lane per (head, key) pair, rows in ascending order.
// grid: x = b * chunks + c, y = group of CR_PAIRS pairs.  The lane of a key at or behind the length reads nothing and writes zeros.
__global__ __launch_bounds__(CR_PAIRS) void cross_bwd_dkv_kernel(const float* q, const float* kc, const float* vc, const float* dO,
                                                                 const float* lse, const float* delta, const int32_t* cond_len, int B,
                                                                 int L, int Te, int H, float* part) {
    const int chunks = cross_chunks(L);
    const int b = (int)(blockIdx.x / (unsigned)chunks), c = (int)(blockIdx.x % (unsigned)chunks);
    const int pr = (int)blockIdx.y * CR_PAIRS + (int)threadIdx.x;           // pair = h * Te + e
    if (pr >= H * Te) return;
    const int h = pr / Te, e = pr - h * Te;
    const int64_t M = (int64_t)B * L;
    float4* dst = reinterpret_cast<float4*>(part + ((int64_t)blockIdx.x * (H * Te) + pr) * 8);
    if (e >= cross_keys(cond_len, b, Te)) {
        dst[0] = make_float4(0.f, 0.f, 0.f, 0.f);
        dst[1] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const float4 kk = *reinterpret_cast<const float4*>(kc + ((int64_t)b * Te + e) * (H * 4) + h * 4);
    const float4 vv = *reinterpret_cast<const float4*>(vc + ((int64_t)b * Te + e) * (H * 4) + h * 4);
    const int r0 = c * CR_ROWS, r1 = min(L, r0 + CR_ROWS);
    const int64_t hm = (int64_t)h * M + (int64_t)b * L;                     // (head, first row of the batch element)
    float dk0 = 0.f, dk1 = 0.f, dk2 = 0.f, dk3 = 0.f, dv0 = 0.f, dv1 = 0.f, dv2 = 0.f, dv3 = 0.f;
    for (int r = r0; r < r1; ++r) {
        const float4 qq = *reinterpret_cast<const float4*>(q + (hm + r) * 4);
        const float4 g = *reinterpret_cast<const float4*>(dO + ((int64_t)b * L + r) * (H * 4) + h * 4);
        const float s = CR_C * fmaf(qq.x, kk.x, fmaf(qq.y, kk.y, fmaf(qq.z, kk.z, qq.w * kk.w)));
        const float p = __builtin_amdgcn_exp2f(s - lse[hm + r]);
        dv0 = fmaf(p, g.x, dv0); dv1 = fmaf(p, g.y, dv1); dv2 = fmaf(p, g.z, dv2); dv3 = fmaf(p, g.w, dv3);
        const float dp = fmaf(g.x, vv.x, fmaf(g.y, vv.y, fmaf(g.z, vv.z, g.w * vv.w)));
        const float ds = p * (dp - delta[hm + r]);
        dk0 = fmaf(ds, qq.x, dk0); dk1 = fmaf(ds, qq.y, dk1); dk2 = fmaf(ds, qq.z, dk2); dk3 = fmaf(ds, qq.w, dk3);
    }
    dst[0] = make_float4(dk0, dk1, dk2, dk3);
    dst[1] = make_float4(dv0, dv1, dv2, dv3);
}

// dkc / dvc rows [B Te][H 4] = the partials of a batch element added in ascending chunk order (overwrites).
// One lane per (b, head, key, component j < 8): consecutive lanes read consecutive floats of a partial.
__global__ __launch_bounds__(256) void cross_bwd_reduce_kernel(const float* part, int B, int L, int Te, int H, float* dkc, float* dvc) {
    const int chunks = cross_chunks(L);
    const int64_t per_b = (int64_t)H * Te * 8;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= per_b * B) return;
    const int b = (int)(i / per_b);
    const int rem = (int)(i - (int64_t)b * per_b);
    const int pr = rem >> 3, j = rem & 7;
    const int h = pr / Te, e = pr - h * Te;
    const float* src = part + (int64_t)b * chunks * per_b + rem;
    float s = 0.f;
    for (int c = 0; c < chunks; ++c) s += src[(int64_t)c * per_b];
    const int64_t dst = ((int64_t)b * Te + e) * (H * 4) + h * 4 + (j & 3);
    if (j < 4) dkc[dst] = 0.5f * s;
    else dvc[dst] = s;
}

}  // namespace gsdd

using namespace gsdd;

static bool cross_sizes_ok(int B, int L, int Te, int H) {
    // (H <= 4096: (head, key) pairs and the rows' pitch stay far inside an int)
    return B > 0 && L > 0 && H > 0 && H <= 4096 && Te >= 1 && Te <= 77;
}

// host copy of the lengths, when the caller has one: every entry in [1, Te] (the kernels clamp what no host has seen)
static int cross_len_check(const char* fn, const int32_t* cond_len_host, int B, int Te) {
    if (cond_len_host == nullptr) return GSDD_OK;
    for (int b = 0; b < B; ++b) {
        if (cond_len_host[b] < 1 || cond_len_host[b] > Te) {
            set_error(std::string(fn) + ": cond_len[" + std::to_string(b) + "] = " + std::to_string(cond_len_host[b]) + " is outside [1, " +
                      std::to_string(Te) + "]");
            return GSDD_E_ARG;
        }
    }
    return GSDD_OK;
}

// cond_len == nullptr: every batch element attends to all Te keys
static int cross_train_launch(const float* q, const float* kc, const float* vc, const int32_t* cond_len, int B, int L, int Te, int H,
                              float* out, float* lse, void* stream) {
    const int64_t n = (int64_t)B * L * H;
    GSDD_CHECK_ARG((n + 255) / 256 < (1ll << 31), "grid too large");
    const dim3 grid((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(cross_train_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, q, kc, vc, cond_len, B, L, Te, H, out, lse);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}

extern "C" int gsdd_d3pm_cross_attention_train(const float* q, const float* kc, const float* vc, int B, int L, int Te, int H,
                                               float* out, float* lse, void* stream) {
    GSDD_CHECK_ARG(q && kc && vc && out && lse, "null pointer");
    GSDD_CHECK_ARG(B > 0 && L > 0 && H > 0 && H <= 4096, "bad sizes");
    GSDD_CHECK_ARG(Te >= 1 && Te <= 77, "Te must be in [1, 77]");
    return cross_train_launch(q, kc, vc, nullptr, B, L, Te, H, out, lse, stream);
}

extern "C" int gsdd_d3pm_cross_attention_train_len(const float* q, const float* kc, const float* vc, const int32_t* cond_len,
                                                   const int32_t* cond_len_host, int B, int L, int Te, int H, float* out, float* lse,
                                                   void* stream) {
    GSDD_CHECK_ARG(q && kc && vc && cond_len && out && lse, "null pointer");
    GSDD_CHECK_ARG(B > 0 && L > 0 && H > 0 && H <= 4096, "bad sizes");
    GSDD_CHECK_ARG(Te >= 1 && Te <= 77, "Te must be in [1, 77]");
    if (cross_len_check(__func__, cond_len_host, B, Te) != GSDD_OK) return GSDD_E_ARG;
    return cross_train_launch(q, kc, vc, cond_len, B, L, Te, H, out, lse, stream);
}

extern "C" int64_t gsdd_d3pm_cross_attention_bwd_workspace_bytes(int B, int L, int Te, int H) {
    if (!cross_sizes_ok(B, L, Te, H)) return 0;
    return cross_delta_bytes((int64_t)B * L, H) + (int64_t)B * cross_chunks(L) * H * Te * 8 * 4;
}

static int cross_bwd_launch(const float* q, const float* kc, const float* vc, const float* o, const float* dO, const float* lse,
                            const int32_t* cond_len, int B, int L, int Te, int H, float* dq, float* dkc, float* dvc, void* workspace,
                            int64_t workspace_bytes, void* stream) {
    GSDD_CHECK_ARG(workspace_bytes >= gsdd_d3pm_cross_attention_bwd_workspace_bytes(B, L, Te, H), "workspace too small");
    const int64_t n = (int64_t)B * L * H;
    const int64_t bc = (int64_t)B * cross_chunks(L);
    const int64_t nred = (int64_t)B * H * Te * 8;
    GSDD_CHECK_ARG((n + 255) / 256 < (1ll << 31) && bc < (1ll << 31) && (nred + 255) / 256 < (1ll << 31), "grid too large");
    hipStream_t st = (hipStream_t)stream;
    float* delta = reinterpret_cast<float*>(workspace);
    float* part = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + cross_delta_bytes((int64_t)B * L, H));
    const dim3 gq((unsigned)((n + 255) / 256)), gkv((unsigned)bc, (unsigned)((H * Te + CR_PAIRS - 1) / CR_PAIRS));
    hipLaunchKernelGGL(cross_bwd_dq_kernel, gq, dim3(256), 0, st, q, kc, vc, o, dO, lse, cond_len, B, L, Te, H, dq, delta);
    GSDD_CHECK_LAUNCH();
    hipLaunchKernelGGL(cross_bwd_dkv_kernel, gkv, dim3(CR_PAIRS), 0, st, q, kc, vc, dO, lse, delta, cond_len, B, L, Te, H, part);
    GSDD_CHECK_LAUNCH();
    hipLaunchKernelGGL(cross_bwd_reduce_kernel, dim3((unsigned)((nred + 255) / 256)), dim3(256), 0, st, part, B, L, Te, H, dkc, dvc);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}

extern "C" int gsdd_d3pm_cross_attention_bwd(const float* q, const float* kc, const float* vc, const float* o, const float* dO,
                                             const float* lse, int B, int L, int Te, int H, float* dq, float* dkc, float* dvc,
                                             void* workspace, int64_t workspace_bytes, void* stream) {
    GSDD_CHECK_ARG(q && kc && vc && o && dO && lse && dq && dkc && dvc && workspace, "null pointer");
    GSDD_CHECK_ARG(B > 0 && L > 0 && H > 0 && H <= 4096, "bad sizes");
    GSDD_CHECK_ARG(Te >= 1 && Te <= 77, "Te must be in [1, 77]");
    return cross_bwd_launch(q, kc, vc, o, dO, lse, nullptr, B, L, Te, H, dq, dkc, dvc, workspace, workspace_bytes, stream);
}

extern "C" int gsdd_d3pm_cross_attention_bwd_len(const float* q, const float* kc, const float* vc, const float* o, const float* dO,
                                                 const float* lse, const int32_t* cond_len, const int32_t* cond_len_host, int B, int L,
                                                 int Te, int H, float* dq, float* dkc, float* dvc, void* workspace,
                                                 int64_t workspace_bytes, void* stream) {
    GSDD_CHECK_ARG(q && kc && vc && o && dO && lse && cond_len && dq && dkc && dvc && workspace, "null pointer");
    GSDD_CHECK_ARG(B > 0 && L > 0 && H > 0 && H <= 4096, "bad sizes");
    GSDD_CHECK_ARG(Te >= 1 && Te <= 77, "Te must be in [1, 77]");
    if (cross_len_check(__func__, cond_len_host, B, Te) != GSDD_OK) return GSDD_E_ARG;
    return cross_bwd_launch(q, kc, vc, o, dO, lse, cond_len, B, L, Te, H, dq, dkc, dvc, workspace, workspace_bytes, stream);
}
