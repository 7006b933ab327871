// Host-side sanitizer driver of the C ABI (tools/host_asan/build.sh): links the host-only ASan / UBSan objects of csrc/*.hip against
// hip_stub.cpp and walks the entry points of include/gsdd.h with
//   (1) valid descriptors at the workload's sizes (fake device pointers: the wrappers must never dereference them on the host) -- every
//       grid / LDS / workspace computation runs under the sanitizers and the stub validates each launch configuration;
//   (2) every workspace contract violated by one byte: the call must return GSDD_E_ARG and launch NOTHING;
//   (3) null pointers, bad sizes, unknown variant / mode values: GSDD_E_ARG, nothing launched;
//   (4) a failing hipFuncSetAttribute: reported as GSDD_E_HIP by that call and retried (successfully) by the next one.
// Exit code 0 = all expectations met and no sanitizer report.  Test infrastructure only.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/gsdd.h"

extern "C" long gsdd_stub_launches();
extern "C" void gsdd_stub_fail_next_set_attribute(long n);

static int g_failed = 0, g_checked = 0;
#define EXPECT(expr, want_rc, want_launch)                                                                                     \
    do {                                                                                                                       \
        const long before_ = gsdd_stub_launches();                                                                             \
        const int rc_ = (expr);                                                                                                \
        const long n_ = gsdd_stub_launches() - before_;                                                                        \
        ++g_checked;                                                                                                           \
        if (rc_ != (want_rc) || ((want_launch) ? n_ <= 0 : n_ != 0)) {                                                         \
            std::fprintf(stderr, "FAIL %s:%d  %s -> rc %d (want %d), %ld launches (want %s) [%s]\n", __FILE__, __LINE__, #expr, rc_, \
                         (int)(want_rc), n_, (want_launch) ? ">0" : "0", gsdd_last_error());                                   \
            ++g_failed;                                                                                                        \
        }                                                                                                                      \
    } while (0)

// distinct fake "device" addresses, 256-byte aligned, in a range no host allocation lives in
static uintptr_t g_next = 0x7000000000ull;
template <class T = float>
static T* devp(size_t bytes = 1 << 20) {
    T* p = reinterpret_cast<T*>(g_next);
    g_next += (bytes + 255) / 256 * 256 + 4096;
    return p;
}

int main() {
    void* st = nullptr;
    const int B = 16, L = 4096, H = 16, K = 4096, T = 100;
    const int64_t M = (int64_t)B * L;

    // ---------------------------------------------------------------- attention (sampler)
    {
        float *q = devp(), *k = devp(), *v = devp(), *out = devp();
        const int64_t need = gsdd_d3pm_attention_workspace_bytes(B, L, H);
        void* ws = devp<void>(need);
        uint64_t* redo = devp<uint64_t>();
        for (int mode = GSDD_ATTN_AUTO; mode <= GSDD_ATTN_KC256; ++mode)
            EXPECT(gsdd_d3pm_attention(q, k, v, B, L, H, out, ws, need, redo, mode, st), GSDD_OK, true);
        EXPECT(gsdd_d3pm_attention(q, nullptr, nullptr, B, L, H, out, ws, need, redo, GSDD_ATTN_A8, st), GSDD_OK, true);
        EXPECT(gsdd_d3pm_attention(q, k, v, B, L, H, out, ws, need - 1, redo, GSDD_ATTN_AUTO, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_attention(q, nullptr, nullptr, B, L, H, out, ws, need - 1, redo, GSDD_ATTN_AUTO, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_attention(q, nullptr, nullptr, B, L, H, out, nullptr, 0, redo, GSDD_ATTN_AUTO, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_attention(q, nullptr, nullptr, B, L, H, out, ws, need, redo, GSDD_ATTN_F32PV, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_attention(q, k, v, B, L, H, out, ws, need, redo, 99, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_attention(q, k, v, B, L, H, out, ws, need, redo, -1, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_attention(q, k, nullptr, B, L, H, out, ws, need, redo, 0, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_attention(q, k, v, 0, L, H, out, ws, need, redo, 0, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_attention(q, k, v, 1 << 20, L, H, out, ws, need, redo, 0, st), GSDD_E_ARG, false);      // grid beyond 2^31
        EXPECT(gsdd_d3pm_attention(q, k, v, 2, 48, H, out, nullptr, 0, nullptr, 0, st), GSDD_OK, true);          // ragged: workspace-free kernel
        EXPECT(gsdd_d3pm_attention(q, k, v, 2, 50, H, out, nullptr, 0, nullptr, 0, st), GSDD_OK, true);          // L % 16 != 0: vector kernel
        // training forward + backward
        float *lse = devp(), *o = devp(), *dO = devp(), *dqkv = devp(), *scratch = devp();
        EXPECT(gsdd_d3pm_attention_train(q, k, v, B, L, H, out, lse, ws, need, GSDD_ATTN_AUTO, st), GSDD_OK, true);
        EXPECT(gsdd_d3pm_attention_train(q, k, v, B, L, H, out, lse, ws, need, GSDD_ATTN_P22, st), GSDD_OK, true);
        EXPECT(gsdd_d3pm_attention_train(q, k, v, B, L, H, out, lse, ws, need, GSDD_ATTN_A8, st), GSDD_OK, true);
        EXPECT(gsdd_d3pm_attention_train(q, k, v, B, L, H, out, lse, nullptr, 0, GSDD_ATTN_AUTO, st), GSDD_OK, true);
        EXPECT(gsdd_d3pm_attention_train(q, k, v, B, L, H, out, lse, ws, need - 1, GSDD_ATTN_AUTO, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_attention_train(q, k, v, B, L, H, out, lse, ws, need, GSDD_ATTN_P11, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_attention_train(q, k, v, B, L, H, out, nullptr, ws, need, GSDD_ATTN_AUTO, st), GSDD_E_ARG, false);
        const int64_t bneed = gsdd_d3pm_attention_bwd_workspace_bytes(B, L, H);
        void* bws = devp<void>(bneed);
        for (int variant = GSDD_ATTN_BWD_AUTO; variant <= GSDD_ATTN_BWD_DEV_LAST; ++variant)
            EXPECT(gsdd_d3pm_attention_bwd(q, k, v, o, dO, lse, B, L, H, dqkv, scratch, bws, bneed, variant, st), GSDD_OK, true);
        EXPECT(gsdd_d3pm_attention_bwd(q, k, v, o, dO, lse, B, L, H, dqkv, scratch, bws, bneed - 1, 0, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_attention_bwd(q, k, v, o, dO, lse, B, L, H, dqkv, nullptr, nullptr, 0, 0, st), GSDD_E_ARG, false);   // vector kernels need scratch
        EXPECT(gsdd_d3pm_attention_bwd(q, k, v, o, dO, lse, B, L, H, dqkv, scratch, nullptr, 0, 0, st), GSDD_OK, true);
        EXPECT(gsdd_d3pm_attention_bwd(q, k, v, o, dO, lse, B, L, H, dqkv, scratch, bws, bneed, 99, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_attention_bwd(q, k, v, o, nullptr, lse, B, L, H, dqkv, scratch, bws, bneed, 0, st), GSDD_E_ARG, false);
    }

    // ---------------------------------------------------------------- cross-attention over Te condition tokens (training)
    {
        const int Te = 22;
        float *q = devp(), *kc = devp(), *vc = devp(), *out = devp(), *lse = devp(), *dO = devp(), *dq = devp(), *dkc = devp(), *dvc = devp();
        EXPECT(gsdd_d3pm_cross_attention_train(q, kc, vc, B, L, Te, H, out, lse, st), GSDD_OK, true);
        EXPECT(gsdd_d3pm_cross_attention_train(q, kc, vc, 3, 1, 77, 1, out, lse, st), GSDD_OK, true);
        EXPECT(gsdd_d3pm_cross_attention_train(q, kc, vc, B, L, 0, H, out, lse, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_cross_attention_train(q, kc, vc, B, L, 78, H, out, lse, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_cross_attention_train(q, kc, vc, 0, L, Te, H, out, lse, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_cross_attention_train(q, kc, vc, B, L, Te, H, out, nullptr, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_cross_attention_train(q, nullptr, vc, B, L, Te, H, out, lse, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_cross_attention_train(nullptr, kc, vc, B, L, Te, H, out, lse, st), GSDD_E_ARG, false);
        const int64_t need = gsdd_d3pm_cross_attention_bwd_workspace_bytes(B, L, Te, H);
        if (need <= 0 || gsdd_d3pm_cross_attention_bwd_workspace_bytes(B, L, 77, H) <= need) {
            std::fprintf(stderr, "FAIL gsdd_d3pm_cross_attention_bwd_workspace_bytes: %lld\n", (long long)need);
            ++g_failed;
        }
        void* ws = devp<void>(need);
        EXPECT(gsdd_d3pm_cross_attention_bwd(q, kc, vc, out, dO, lse, B, L, Te, H, dq, dkc, dvc, ws, need, st), GSDD_OK, true);
        EXPECT(gsdd_d3pm_cross_attention_bwd(q, kc, vc, out, dO, lse, 3, 1, 1, 1, dq, dkc, dvc, ws, need, st), GSDD_OK, true);
        EXPECT(gsdd_d3pm_cross_attention_bwd(q, kc, vc, out, dO, lse, B, L, Te, H, dq, dkc, dvc, ws, need - 1, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_cross_attention_bwd(q, kc, vc, out, dO, lse, B, L, Te, H, dq, dkc, dvc, nullptr, need, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_cross_attention_bwd(q, kc, vc, out, dO, lse, B, L, 0, H, dq, dkc, dvc, ws, need, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_cross_attention_bwd(q, kc, vc, out, dO, lse, B, L, 78, H, dq, dkc, dvc, ws, need, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_cross_attention_bwd(q, kc, vc, out, nullptr, lse, B, L, Te, H, dq, dkc, dvc, ws, need, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_cross_attention_bwd(q, kc, vc, out, dO, nullptr, B, L, Te, H, dq, dkc, dvc, ws, need, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_cross_attention_bwd(q, kc, vc, out, dO, lse, B, L, Te, H, nullptr, dkc, dvc, ws, need, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_cross_attention_bwd(q, kc, vc, out, dO, lse, B, L, Te, H, dq, nullptr, dvc, ws, need, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_cross_attention_bwd(q, kc, vc, out, dO, lse, B, L, Te, H, dq, dkc, nullptr, ws, need, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_cross_attention_bwd(q, kc, vc, out, dO, lse, B, 0, Te, H, dq, dkc, dvc, ws, need, st), GSDD_E_ARG, false);
        // the same three with a condition length per batch element: a device array plus an optional host copy that is range-checked
        {
            const int32_t* len = devp<int32_t>();
            std::vector<int32_t> len_h(B);
            for (int b = 0; b < B; ++b) len_h[b] = 1 + (b * 5) % Te;
            len_h[1] = Te;
            EXPECT(gsdd_d3pm_cross_attention_len(q, kc, vc, len, len_h.data(), B, L, Te, H, out, st), GSDD_OK, true);
            EXPECT(gsdd_d3pm_cross_attention_len(q, kc, vc, len, nullptr, B, L, Te, H, out, st), GSDD_OK, true);
            EXPECT(gsdd_d3pm_cross_attention_train_len(q, kc, vc, len, len_h.data(), B, L, Te, H, out, lse, st), GSDD_OK, true);
            EXPECT(gsdd_d3pm_cross_attention_train_len(q, kc, vc, len, nullptr, B, L, Te, H, out, lse, st), GSDD_OK, true);
            EXPECT(gsdd_d3pm_cross_attention_bwd_len(q, kc, vc, out, dO, lse, len, len_h.data(), B, L, Te, H, dq, dkc, dvc, ws, need, st), GSDD_OK, true);
            EXPECT(gsdd_d3pm_cross_attention_bwd_len(q, kc, vc, out, dO, lse, len, nullptr, B, L, Te, H, dq, dkc, dvc, ws, need, st), GSDD_OK, true);
            EXPECT(gsdd_d3pm_cross_attention_bwd_len(q, kc, vc, out, dO, lse, len, len_h.data(), B, L, Te, H, dq, dkc, dvc, ws, need - 1, st), GSDD_E_ARG, false);
            // null pointers (the host copy alone may be null)
            EXPECT(gsdd_d3pm_cross_attention_len(q, kc, vc, nullptr, len_h.data(), B, L, Te, H, out, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_cross_attention_len(q, kc, vc, len, len_h.data(), B, L, Te, H, nullptr, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_cross_attention_len(q, nullptr, vc, len, len_h.data(), B, L, Te, H, out, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_cross_attention_train_len(q, kc, vc, nullptr, nullptr, B, L, Te, H, out, lse, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_cross_attention_train_len(q, kc, vc, len, nullptr, B, L, Te, H, out, nullptr, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_cross_attention_bwd_len(q, kc, vc, out, dO, lse, nullptr, nullptr, B, L, Te, H, dq, dkc, dvc, ws, need, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_cross_attention_bwd_len(q, kc, vc, out, dO, lse, len, nullptr, B, L, Te, H, dq, dkc, dvc, nullptr, need, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_cross_attention_bwd_len(q, kc, vc, out, dO, lse, len, nullptr, B, L, Te, H, dq, nullptr, dvc, ws, need, st), GSDD_E_ARG, false);
            // Te out of range
            EXPECT(gsdd_d3pm_cross_attention_len(q, kc, vc, len, nullptr, B, L, 0, H, out, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_cross_attention_train_len(q, kc, vc, len, nullptr, B, L, 78, H, out, lse, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_cross_attention_bwd_len(q, kc, vc, out, dO, lse, len, nullptr, B, L, 78, H, dq, dkc, dvc, ws, need, st), GSDD_E_ARG, false);
            // host lengths 0 and Te + 1: refused before the launch, the message names index and value
            for (int32_t bad : {(int32_t)0, (int32_t)(Te + 1)}) {
                len_h[B - 1] = bad;
                EXPECT(gsdd_d3pm_cross_attention_len(q, kc, vc, len, len_h.data(), B, L, Te, H, out, st), GSDD_E_ARG, false);
                EXPECT(gsdd_d3pm_cross_attention_train_len(q, kc, vc, len, len_h.data(), B, L, Te, H, out, lse, st), GSDD_E_ARG, false);
                EXPECT(gsdd_d3pm_cross_attention_bwd_len(q, kc, vc, out, dO, lse, len, len_h.data(), B, L, Te, H, dq, dkc, dvc, ws, need, st), GSDD_E_ARG, false);
                char want[64];
                std::snprintf(want, sizeof want, "cond_len[%d] = %d", B - 1, (int)bad);
                if (std::strstr(gsdd_last_error(), want) == nullptr) {
                    std::fprintf(stderr, "FAIL the message does not name index and value: %s\n", gsdd_last_error());
                    ++g_failed;
                }
            }
        }
        // LayerNorm rows of any width (the text tower's per-token features)
        EXPECT(gsdd_ln_apply(q, kc, vc, dO, 16 * 22, 512, out, st), GSDD_OK, true);
        EXPECT(gsdd_ln_apply(q, kc, vc, dO, 16 * 22, 510, out, st), GSDD_E_ARG, false);
        EXPECT(gsdd_ln_apply(q, nullptr, vc, dO, 16 * 22, 512, out, st), GSDD_E_ARG, false);
        EXPECT(gsdd_ln_apply(q, kc, vc, dO, 0, 512, out, st), GSDD_E_ARG, false);
    }

    // ---------------------------------------------------------------- fused layer
    {
        gsdd_layer_desc d;
        std::memset(&d, 0, sizeof d);
        d.y = devp(); d.x = devp(); d.M = 2 * M; d.L = L; d.n_embd = 64; d.hidden = 256; d.cvec = devp();
        d.wproj = devp(); d.bproj = devp(); d.ln2_g = devp(); d.ln2_b = devp(); d.w1 = devp(); d.b1 = devp(); d.w2 = devp(); d.b2 = devp();
        d.ada = devp(); d.t2 = devp<int64_t>(); d.wqkv = devp(); d.bqkv = devp(); d.qkv = devp();
        EXPECT(gsdd_d3pm_layer(&d, st), GSDD_E_ARG, false);                          // no fragment images at all
        d.layer_h2 = devp<void>(); d.wqkv_h2 = devp<void>();
        EXPECT(gsdd_d3pm_layer(&d, st), GSDD_OK, true);
        d.variant = GSDD_LAYER_X3P;
        EXPECT(gsdd_d3pm_layer(&d, st), GSDD_E_ARG, false);                          // asks for the bf16x3 kernel, has only the f16 images
        d.w2_x3 = devp<void>(); d.wqkv_x3 = devp<void>();
        EXPECT(gsdd_d3pm_layer(&d, st), GSDD_OK, true);
        d.variant = 1;
        EXPECT(gsdd_d3pm_layer(&d, st), GSDD_E_ARG, false);                          // the removed split-on-the-fly kernel's old number
        d.variant = GSDD_LAYER_AUTO;
        const int64_t need = gsdd_d3pm_attention_workspace_bytes(2 * B, L, 16);
        d.kv_img = devp<void>(need); d.kv_img_bytes = need;
        d.range_flag = devp<int>();
        EXPECT(gsdd_d3pm_layer(&d, st), GSDD_OK, true);
        d.kv_img_bytes = need - 1;
        EXPECT(gsdd_d3pm_layer(&d, st), GSDD_E_ARG, false);
        d.kv_img_bytes = need;
        d.L = 4090;
        EXPECT(gsdd_d3pm_layer(&d, st), GSDD_E_ARG, false);                          // images need L % 32 == 0
        d.L = L; d.n_embd = 128;
        EXPECT(gsdd_d3pm_layer(&d, st), GSDD_E_ARG, false);
        d.n_embd = 64;
        const float* keep = d.y; d.y = nullptr;                                       // q|k|v stage only (block 0)
        EXPECT(gsdd_d3pm_layer(&d, st), GSDD_OK, true);
        d.qkv = nullptr;
        EXPECT(gsdd_d3pm_layer(&d, st), GSDD_E_ARG, false);
        d.y = keep;
        EXPECT(gsdd_d3pm_layer(nullptr, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_logits(devp(), 2 * M, 64, devp(), devp(), devp(), devp(), K, devp(), st), GSDD_OK, true);
        EXPECT(gsdd_d3pm_logits(devp(), 2 * M, 64, devp(), devp(), devp(), devp(), K + 2, devp(), st), GSDD_E_ARG, false);
        // a failing per-device attribute call is reported and retried (first use of the bf16x3 q|k|v-only instantiation set)
        gsdd_stub_fail_next_set_attribute(1);
        EXPECT(gsdd_rows_linear(devp(), M, 64, devp<void>(), 256, devp(), nullptr, 0, nullptr, devp(), 0, st), GSDD_E_HIP, false);
        EXPECT(gsdd_rows_linear(devp(), M, 64, devp<void>(), 256, devp(), nullptr, 0, nullptr, devp(), 0, st), GSDD_OK, true);
        EXPECT(gsdd_rows_linear(devp(), M, 64, devp<void>(), 320, devp(), nullptr, 0, nullptr, devp(), 0, st), GSDD_E_ARG, false);
    }

    // ---------------------------------------------------------------- posterior step / q_sample / training objective
    {
        gsdd_step_desc d;
        std::memset(&d, 0, sizeof d);
        d.logits_c = devp(); d.logits_u = devp(); d.tok_in = devp<int64_t>(); d.tok_out = devp<int64_t>();
        d.B = B; d.L = L; d.K = K; d.T = T; d.guidance = 2.f;
        const float* sched[8];
        for (int i = 0; i < 8; ++i) d.sched[i] = sched[i] = devp();
        d.t_dev = devp<int64_t>(); d.stream_dev = devp<int64_t>(); d.seed = 1;
        EXPECT(gsdd_d3pm_step(&d, st), GSDD_OK, true);
        d.occupancy = 3;
        EXPECT(gsdd_d3pm_step(&d, st), GSDD_OK, true);
        d.occupancy = 7;
        EXPECT(gsdd_d3pm_step(&d, st), GSDD_E_ARG, false);
        d.occupancy = 0;
        d.post_skip = 3;
        EXPECT(gsdd_d3pm_step(&d, st), GSDD_OK, true);
        d.post_skip = -1;
        EXPECT(gsdd_d3pm_step(&d, st), GSDD_E_ARG, false);
        d.post_skip = 0;
        d.trunc_rate = 0.86f;                                                    // top-r truncation: the truncated kernel family
        EXPECT(gsdd_d3pm_step(&d, st), GSDD_OK, true);
        for (float bad : {1.f, -0.5f, 1.5f}) { d.trunc_rate = bad; EXPECT(gsdd_d3pm_step(&d, st), GSDD_E_ARG, false); }
        d.trunc_rate = 0.f;
        d.known = devp<uint8_t>(); d.x_known = devp<int64_t>();                 // known positions: the masked kernel families
        for (int mode : {0, 1}) { d.known_mode = mode; EXPECT(gsdd_d3pm_step(&d, st), GSDD_OK, true); }
        d.trunc_rate = 0.86f;
        EXPECT(gsdd_d3pm_step(&d, st), GSDD_OK, true);
        d.trunc_rate = 0.f;
        for (int bad : {-1, 2}) { d.known_mode = bad; EXPECT(gsdd_d3pm_step(&d, st), GSDD_E_ARG, false); }
        d.known_mode = 0;
        d.x_known = nullptr;
        EXPECT(gsdd_d3pm_step(&d, st), GSDD_E_ARG, false);
        d.x_known = devp<int64_t>(); d.post_dbg = devp();                         // the masked families carry no hooks
        EXPECT(gsdd_d3pm_step(&d, st), GSDD_E_ARG, false);
        d.post_dbg = nullptr; d.known = nullptr; d.known_mode = 5;               // without a mask the other two fields are not looked at
        EXPECT(gsdd_d3pm_step(&d, st), GSDD_OK, true);
        d.x_known = nullptr; d.known_mode = 0;
        EXPECT(gsdd_advance_floor(devp<int64_t>(), B, -4, 0, devp<int64_t>(), 1, st), GSDD_OK, true);
        EXPECT(gsdd_advance_floor(devp<int64_t>(), -1, -4, 0, devp<int64_t>(), 1, st), GSDD_E_ARG, false);
        for (int k : {4, 32, 768, 1024, 2048, 4092, 8192}) { d.K = k; EXPECT(gsdd_d3pm_step(&d, st), GSDD_OK, true); }
        d.K = 8196;
        EXPECT(gsdd_d3pm_step(&d, st), GSDD_E_ARG, false);
        d.K = 30;
        EXPECT(gsdd_d3pm_step(&d, st), GSDD_E_ARG, false);
        d.K = K; d.sched[3] = nullptr;
        EXPECT(gsdd_d3pm_step(&d, st), GSDD_E_ARG, false);
        EXPECT(gsdd_d3pm_q_sample(devp<int64_t>(), devp<int64_t>(), B, L, K, T, sched, devp<int64_t>(), 1, devp<int64_t>(), 0, st), GSDD_OK, true);
        {   // forward jump (RePaint's resampling): every class width, in place, with and without a hold mask; bad arguments
            gsdd_jump_desc j;
            std::memset(&j, 0, sizeof j);
            j.tok_in = devp<int64_t>(); j.tok_out = devp<int64_t>();
            j.B = B; j.L = L; j.K = K; j.T = T; j.table = devp(); j.jump = 10;
            j.t_dev = devp<int64_t>(); j.stream_dev = devp<int64_t>(); j.seed = 1; j.row0 = 1000;
            EXPECT(gsdd_d3pm_forward_jump(&j, st), GSDD_OK, true);
            j.hold = devp<uint8_t>(); j.tok_out = const_cast<int64_t*>(j.tok_in);
            EXPECT(gsdd_d3pm_forward_jump(&j, st), GSDD_OK, true);
            for (int k : {4, 32, 768, 1024, 2048, 4092, 8192}) { j.K = k; EXPECT(gsdd_d3pm_forward_jump(&j, st), GSDD_OK, true); }
            for (int bad : {0, 2, 30, 8196, -4}) { j.K = bad; EXPECT(gsdd_d3pm_forward_jump(&j, st), GSDD_E_ARG, false); }
            j.K = K;
            for (int bad : {0, -1, T + 1}) { j.jump = bad; EXPECT(gsdd_d3pm_forward_jump(&j, st), GSDD_E_ARG, false); }
            j.jump = 1;
            EXPECT(gsdd_d3pm_forward_jump(&j, st), GSDD_OK, true);
            j.table = nullptr;
            EXPECT(gsdd_d3pm_forward_jump(&j, st), GSDD_E_ARG, false);
            j.table = devp(); j.tok_in = nullptr;
            EXPECT(gsdd_d3pm_forward_jump(&j, st), GSDD_E_ARG, false);
            j.tok_in = devp<int64_t>(); j.tok_out = nullptr;
            EXPECT(gsdd_d3pm_forward_jump(&j, st), GSDD_E_ARG, false);
            j.tok_out = devp<int64_t>(); j.t_dev = nullptr;
            EXPECT(gsdd_d3pm_forward_jump(&j, st), GSDD_E_ARG, false);
            j.t_dev = devp<int64_t>(); j.stream_dev = nullptr;
            EXPECT(gsdd_d3pm_forward_jump(&j, st), GSDD_E_ARG, false);
            j.stream_dev = devp<int64_t>(); j.B = 0;
            EXPECT(gsdd_d3pm_forward_jump(&j, st), GSDD_E_ARG, false);
            j.B = B;
            EXPECT(gsdd_d3pm_forward_jump(nullptr, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_forward_jump(&j, st), GSDD_OK, true);
        }
        {   // composed guidance: every class width and condition count, in place and into a buffer of its own; bad arguments
            gsdd_compose_desc c;
            std::memset(&c, 0, sizeof c);
            float* lg = devp(1 << 20);
            c.logits = lg; c.weights = devp(); c.out = devp(); c.n_cond = 2; c.B = 2; c.L = 3; c.K = 8;
            const size_t blk = (size_t)c.B * c.L * c.K;
            EXPECT(gsdd_d3pm_compose(&c, st), GSDD_OK, true);
            c.out = lg;                                                  // block 0: in place
            EXPECT(gsdd_d3pm_compose(&c, st), GSDD_OK, true);
            c.out = lg + 3 * blk;                                        // right behind the last block
            EXPECT(gsdd_d3pm_compose(&c, st), GSDD_OK, true);
            for (size_t off : {blk, 2 * blk, (size_t)4, 3 * blk - 4}) { c.out = lg + off; EXPECT(gsdd_d3pm_compose(&c, st), GSDD_E_ARG, false); }
            c.out = lg + 1;                                              // not 16-byte aligned
            EXPECT(gsdd_d3pm_compose(&c, st), GSDD_E_ARG, false);
            c.out = lg;
            for (int n : {1, 3, 4}) { c.n_cond = n; EXPECT(gsdd_d3pm_compose(&c, st), GSDD_OK, true); }
            for (int bad : {0, -1, 5}) { c.n_cond = bad; EXPECT(gsdd_d3pm_compose(&c, st), GSDD_E_ARG, false); }
            c.n_cond = 2;
            for (int k : {4, 256, 1020, 2048, 4092, 4096, 8192}) { c.K = k; EXPECT(gsdd_d3pm_compose(&c, st), GSDD_OK, true); }
            for (int bad : {0, 2, 30, 8196, -4}) { c.K = bad; EXPECT(gsdd_d3pm_compose(&c, st), GSDD_E_ARG, false); }
            c.K = 8; c.logits = nullptr;
            EXPECT(gsdd_d3pm_compose(&c, st), GSDD_E_ARG, false);
            c.logits = lg; c.weights = nullptr;
            EXPECT(gsdd_d3pm_compose(&c, st), GSDD_E_ARG, false);
            c.weights = devp(); c.out = nullptr;
            EXPECT(gsdd_d3pm_compose(&c, st), GSDD_E_ARG, false);
            c.out = lg; c.B = 0;
            EXPECT(gsdd_d3pm_compose(&c, st), GSDD_E_ARG, false);
            c.B = 2;
            EXPECT(gsdd_d3pm_compose(nullptr, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_compose(&c, st), GSDD_OK, true);
        }
        {   // the training step's gradient reductions, in the fast form and in the reproducible one (gsdd_set_deterministic)
            float *dh = devp(1 << 25), *xr = devp(1 << 25), *stats = devp(), *gam = devp(), *dxo = devp(1 << 25), *dg = devp(), *dbt = devp();
            float *dW = devp(), *dbias = devp(), *osum = devp(), *dtab = devp(), *emb = devp(), *wad = devp(), *demb = devp(), *dpos = devp(1 << 21);
            int64_t *sel = devp<int64_t>(), *tokp = devp<int64_t>();
            EXPECT(gsdd_set_deterministic(0), 0, false);
            for (int det = 0; det < 2; ++det) {
                EXPECT(gsdd_set_deterministic(det), det ? 0 : 0, false);
                EXPECT(gsdd_ln_bwd(dh, xr, stats, gam, sel, 128, L, M, 64, nullptr, dxo, dg, dbt, 128, 1, st), GSDD_OK, true);       // AdaLN: per-batch slots
                EXPECT(gsdd_ln_bwd(dh, xr, stats, gam, sel, 128, 40, 160, 64, dh, dxo, dg, dbt, 128, 1, st), GSDD_OK, true);        // L % 16 != 0
                EXPECT(gsdd_ln_bwd(dh, xr, stats, gam, nullptr, 0, L, M, 64, nullptr, dxo, dg, dbt, 64, 0, st), GSDD_OK, true);     // affine LN
                EXPECT(gsdd_ln_bwd(dh, xr, stats, gam, nullptr, 0, L, M, 64, nullptr, dxo, nullptr, nullptr, 64, 0, st), GSDD_OK, true);
                EXPECT(gsdd_wgrad(dh, 64, xr, 64, M, 64, 64, dW, dbias, st), GSDD_OK, true);
                EXPECT(gsdd_wgrad(dh, 256, xr, 64, 160, 256, 64, dW, nullptr, st), GSDD_OK, true);
                EXPECT(gsdd_colsum(dh, 64, M, 64, osum, st), GSDD_OK, true);
                EXPECT(gsdd_batch_rowsum(dh, B, L, 64, osum, st), GSDD_OK, true);
                EXPECT(gsdd_d3pm_embed_bwd(dh, tokp, B, L, 64, K + 1, demb, dpos, st), GSDD_OK, true);
                EXPECT(gsdd_adaln_bwd(dtab, sel, B, 64, emb, wad, demb, dW, dbias, st), GSDD_OK, true);
                EXPECT(gsdd_wgrad(dh, 64, xr, 64, 0, 64, 64, dW, dbias, st), GSDD_E_ARG, false);
                EXPECT(gsdd_ln_bwd(dh, xr, stats, gam, sel, 128, L, M, 64, nullptr, dxo, dg, nullptr, 128, 1, st), GSDD_E_ARG, false);
                EXPECT(gsdd_d3pm_embed_bwd(dh, nullptr, B, L, 64, K + 1, demb, dpos, st), GSDD_E_ARG, false);
            }
            EXPECT(gsdd_set_deterministic(0), 1, false);             // returns the previous setting
            EXPECT(gsdd_set_deterministic(0), 0, false);
        }
        {   // classifier-free training: condition dropout (drawn and with a mask) and the null embedding's gradient; bad arguments
            const int Te = 22, C = 512, D = 64;
            float *cond = devp(), *null_rows = devp(), *out = devp();
            int64_t* sid = devp<int64_t>();
            uint8_t *din = devp<uint8_t>(), *dout = devp<uint8_t>();
            EXPECT(gsdd_cond_dropout(cond, null_rows, B, Te, C, 0.1f, 21, sid, 1000, nullptr, out, dout, st), GSDD_OK, true);
            EXPECT(gsdd_cond_dropout(cond, null_rows, B, Te, C, 0.f, 21, nullptr, 0, din, out, dout, st), GSDD_OK, true);
            EXPECT(gsdd_cond_dropout(cond, null_rows, 5, 77, C, 1.f, 21, sid, (int64_t)1 << 33, nullptr, out, dout, st), GSDD_OK, true);
            EXPECT(gsdd_cond_dropout(cond, null_rows, 1, 1, 4, 0.5f, 21, sid, 0, nullptr, out, dout, st), GSDD_OK, true);
            EXPECT(gsdd_cond_dropout(nullptr, null_rows, B, Te, C, 0.1f, 21, sid, 0, nullptr, out, dout, st), GSDD_E_ARG, false);
            EXPECT(gsdd_cond_dropout(cond, nullptr, B, Te, C, 0.1f, 21, sid, 0, nullptr, out, dout, st), GSDD_E_ARG, false);
            EXPECT(gsdd_cond_dropout(cond, null_rows, B, Te, C, 0.1f, 21, sid, 0, nullptr, nullptr, dout, st), GSDD_E_ARG, false);
            EXPECT(gsdd_cond_dropout(cond, null_rows, B, Te, C, 0.1f, 21, sid, 0, nullptr, out, nullptr, st), GSDD_E_ARG, false);
            EXPECT(gsdd_cond_dropout(cond, null_rows, B, Te, C, 0.1f, 21, nullptr, 0, nullptr, out, dout, st), GSDD_E_ARG, false);   // a draw without sid
            for (int bad : {0, -1, 78}) EXPECT(gsdd_cond_dropout(cond, null_rows, B, bad, C, 0.1f, 21, sid, 0, nullptr, out, dout, st), GSDD_E_ARG, false);
            for (int bad : {0, -4, 6, 510}) EXPECT(gsdd_cond_dropout(cond, null_rows, B, Te, bad, 0.1f, 21, sid, 0, nullptr, out, dout, st), GSDD_E_ARG, false);
            for (float bad : {-0.1f, 1.5f, NAN}) EXPECT(gsdd_cond_dropout(cond, null_rows, B, Te, C, bad, 21, sid, 0, nullptr, out, dout, st), GSDD_E_ARG, false);
            EXPECT(gsdd_cond_dropout(cond, null_rows, 0, Te, C, 0.1f, 21, sid, 0, nullptr, out, dout, st), GSDD_E_ARG, false);
            EXPECT(gsdd_cond_dropout(cond, null_rows, B, Te, C, 0.1f, 21, sid, -1, nullptr, out, dout, st), GSDD_E_ARG, false);
            EXPECT(gsdd_cond_dropout(cond, null_rows, B, Te, C, 0.1f, 21, sid, 0, nullptr, cond, dout, st), GSDD_E_ARG, false);      // out == cond
            EXPECT(gsdd_cond_dropout(cond, null_rows, B, Te, C, 0.1f, 21, sid, 0, nullptr, cond + Te * C, dout, st), GSDD_E_ARG, false);   // overlap
            EXPECT(gsdd_cond_dropout(cond, null_rows, B, Te, C, 0.1f, 21, sid, 0, nullptr, null_rows, dout, st), GSDD_E_ARG, false);
            EXPECT(gsdd_cond_dropout(cond + 1, null_rows, B, Te, C, 0.1f, 21, sid, 0, nullptr, out, dout, st), GSDD_E_ARG, false);   // not 16-byte aligned
            float *dk = devp(), *dv = devp(), *wk = devp(), *wv = devp(), *dnull = devp();
            EXPECT(gsdd_cond_null_grad(dk, dv, dout, wk, wv, B, Te, D, C, dnull, st), GSDD_OK, true);
            EXPECT(gsdd_cond_null_grad(nullptr, dv, dout, nullptr, wv, B, 1, D, C, dnull, st), GSDD_OK, true);                        // one token: no key term
            EXPECT(gsdd_cond_null_grad(dk, dv, dout, wk, wv, 3, 77, 4096, 20, dnull, st), GSDD_OK, true);
            EXPECT(gsdd_cond_null_grad(dk, dv, dout, nullptr, wv, B, Te, D, C, dnull, st), GSDD_E_ARG, false);
            EXPECT(gsdd_cond_null_grad(nullptr, dv, dout, wk, wv, B, Te, D, C, dnull, st), GSDD_E_ARG, false);
            EXPECT(gsdd_cond_null_grad(dk, nullptr, dout, wk, wv, B, Te, D, C, dnull, st), GSDD_E_ARG, false);
            EXPECT(gsdd_cond_null_grad(dk, dv, nullptr, wk, wv, B, Te, D, C, dnull, st), GSDD_E_ARG, false);
            EXPECT(gsdd_cond_null_grad(dk, dv, dout, wk, nullptr, B, Te, D, C, dnull, st), GSDD_E_ARG, false);
            EXPECT(gsdd_cond_null_grad(dk, dv, dout, wk, wv, B, Te, D, C, nullptr, st), GSDD_E_ARG, false);
            for (int bad : {0, -1, 78}) EXPECT(gsdd_cond_null_grad(dk, dv, dout, wk, wv, B, bad, D, C, dnull, st), GSDD_E_ARG, false);
            for (int bad : {0, -1, 4097}) EXPECT(gsdd_cond_null_grad(dk, dv, dout, wk, wv, B, Te, bad, C, dnull, st), GSDD_E_ARG, false);
            EXPECT(gsdd_cond_null_grad(dk, dv, dout, wk, wv, 0, Te, D, C, dnull, st), GSDD_E_ARG, false);
            EXPECT(gsdd_cond_null_grad(dk, dv, dout, wk, wv, B, Te, D, 0, dnull, st), GSDD_E_ARG, false);
        }
        {   // purity-prior step: scores + candidates, selection, plan counter
            gsdd_purity_desc p;
            std::memset(&p, 0, sizeof p);
            p.logits_c = devp(); p.logits_u = devp(); p.B = B; p.L = L; p.K = K; p.guidance = 2.f; p.prior_rule = 2; p.seed = 1;
            p.stream_dev = devp<int64_t>(); p.score = devp(); p.smax = devp(); p.cand = devp<int64_t>();
            EXPECT(gsdd_d3pm_purity_step(&p, st), GSDD_OK, true);                // one pass
            p.prior_weight = 1.f;
            EXPECT(gsdd_d3pm_purity_step(&p, st), GSDD_OK, true);                // scores, smax, draw
            p.recon_dbg = devp(); p.prob_dbg = devp(); p.score_dbg = devp();
            EXPECT(gsdd_d3pm_purity_step(&p, st), GSDD_OK, true);                // the hooked instantiation
            p.trunc_rate = 0.86f;
            EXPECT(gsdd_d3pm_purity_step(&p, st), GSDD_OK, true);                // hooked and truncated
            p.recon_dbg = p.prob_dbg = p.score_dbg = nullptr;
            EXPECT(gsdd_d3pm_purity_step(&p, st), GSDD_OK, true);
            p.trunc_rate = 1.f;
            EXPECT(gsdd_d3pm_purity_step(&p, st), GSDD_E_ARG, false);
            p.trunc_rate = 0.f;
            p.prior_rule = 1; p.logits_u = nullptr;
            for (int k : {4, 32, 768, 1024, 2048, 4092, 8192}) { p.K = k; EXPECT(gsdd_d3pm_purity_step(&p, st), GSDD_OK, true); }
            p.K = 30;
            EXPECT(gsdd_d3pm_purity_step(&p, st), GSDD_E_ARG, false);
            p.K = K; p.prior_rule = 0;
            EXPECT(gsdd_d3pm_purity_step(&p, st), GSDD_E_ARG, false);
            p.prior_rule = 2; p.prior_weight = -1.f;
            EXPECT(gsdd_d3pm_purity_step(&p, st), GSDD_E_ARG, false);
            p.prior_weight = 0.f; p.smax = nullptr;
            EXPECT(gsdd_d3pm_purity_step(&p, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_purity_step(nullptr, st), GSDD_E_ARG, false);
            gsdd_purity_select_desc s;
            std::memset(&s, 0, sizeof s);
            s.tok_in = devp<int64_t>(); s.tok_out = devp<int64_t>(); s.cand = devp<int64_t>(); s.score = devp(); s.smax = devp();
            s.B = B; s.L = L; s.K = K; s.prior_rule = 2; s.n_dev = devp<int64_t>(); s.seed = 1; s.stream_dev = devp<int64_t>();
            s.stream_add = 1; s.row0 = 3 * (int64_t)L;
            EXPECT(gsdd_d3pm_purity_select(&s, st), GSDD_OK, true);
            s.prior_rule = 1; s.score = nullptr; s.smax = nullptr;
            EXPECT(gsdd_d3pm_purity_select(&s, st), GSDD_OK, true);
            s.prior_rule = 2;
            EXPECT(gsdd_d3pm_purity_select(&s, st), GSDD_E_ARG, false);            // rule 2 needs the scores
            s.prior_rule = 1; s.row0 = 5;
            EXPECT(gsdd_d3pm_purity_select(&s, st), GSDD_E_ARG, false);            // row0 is a multiple of L
            s.row0 = 0; s.L = 4097;
            EXPECT(gsdd_d3pm_purity_select(&s, st), GSDD_E_ARG, false);            // one sample is sorted in LDS
            s.L = L; s.n_dev = nullptr;
            EXPECT(gsdd_d3pm_purity_select(&s, st), GSDD_E_ARG, false);
            EXPECT(gsdd_advance_plan(devp<int64_t>(), devp<int64_t>(), devp<int64_t>(), 42, devp<int64_t>(), B, devp<int64_t>(),
                                     devp<int64_t>(), 2, st), GSDD_OK, true);
            EXPECT(gsdd_advance_plan(devp<int64_t>(), devp<int64_t>(), devp<int64_t>(), 0, devp<int64_t>(), B, devp<int64_t>(),
                                     devp<int64_t>(), 2, st), GSDD_E_ARG, false);
            EXPECT(gsdd_advance_plan(devp<int64_t>(), nullptr, devp<int64_t>(), 42, devp<int64_t>(), B, devp<int64_t>(), nullptr, 2, st),
                   GSDD_E_ARG, false);
        }
        gsdd_train_desc t;
        std::memset(&t, 0, sizeof t);
        t.logits = devp(); t.x0 = devp<int64_t>(); t.xt = devp<int64_t>(); t.t_dev = devp<int64_t>(); t.pt = devp();
        t.B = B; t.L = L; t.K = K; t.T = T;
        for (int i = 0; i < 8; ++i) t.sched[i] = sched[i];
        t.mask_weight[0] = t.mask_weight[1] = 1.f; t.aux_weight = 5e-4f; t.adaptive_aux = 1;
        t.kl = devp(); t.nll = devp(); t.aux = devp(); t.x0_recon = devp<int64_t>(); t.xt1_recon = devp<int64_t>();
        t.Lt_history = devp(); t.Lt_count = devp(); t.loss = devp(); t.per_sample = devp();
        EXPECT(gsdd_d3pm_train_loss(&t, st), GSDD_OK, true);
        EXPECT(gsdd_d3pm_train_loss_grad(&t, devp(), st), GSDD_OK, true);
        EXPECT(gsdd_d3pm_train_loss_bwd(&t, devp(), st), GSDD_OK, true);
        t.K = 8192;                                                          // J = 32: the 128 KB LDS attribute is requested here only
        EXPECT(gsdd_d3pm_train_loss_grad(&t, devp(), st), GSDD_OK, true);
        t.K = K;
        EXPECT(gsdd_d3pm_train_loss_grad(&t, nullptr, st), GSDD_E_ARG, false);
    }

    // ---------------------------------------------------------------- VQ-VAE pieces with workspaces
    {
        const int64_t Mz = 64 * 4096;
        const int64_t need = gsdd_nearest_code_workspace_bytes(4096);
        EXPECT(gsdd_nearest_code(devp(), Mz, 128, devp(), 4096, devp<int64_t>(), devp(), devp<void>(), need, st), GSDD_OK, true);
        EXPECT(gsdd_nearest_code(devp(), Mz, 128, devp(), 4096, devp<int64_t>(), devp(), devp<void>(), need - 1, st), GSDD_E_ARG, false);
        EXPECT(gsdd_nearest_code(devp(), Mz, 128, devp(), 4096, devp<int64_t>(), nullptr, nullptr, 0, st), GSDD_OK, true);     // vector kernel
        EXPECT(gsdd_nearest_code(devp(), Mz, 130, devp(), 4096, devp<int64_t>(), nullptr, nullptr, 0, st), GSDD_E_ARG, false);
        const int64_t bn = gsdd_bn_train_workspace_bytes(Mz, 256);
        EXPECT(gsdd_bn_train(devp(), Mz, 256, devp(), devp(), 1e-5f, 0.1f, devp(), devp(), devp(), devp(), devp(), devp<void>(), bn, st), GSDD_OK, true);
        EXPECT(gsdd_bn_train(devp(), Mz, 256, devp(), devp(), 1e-5f, 0.1f, devp(), devp(), devp(), devp(), devp(), devp<void>(), bn - 1, st), GSDD_E_ARG, false);
        const int64_t bb = gsdd_bn_relu_bwd_workspace_bytes(Mz, 256);
        EXPECT(gsdd_bn_relu_bwd(devp(), devp(), Mz, 256, devp(), devp(), devp(), nullptr, devp(), devp(), devp(), devp<void>(), bb, st), GSDD_OK, true);
        EXPECT(gsdd_bn_relu_bwd(devp(), devp(), Mz, 256, devp(), devp(), devp(), nullptr, devp(), devp(), devp(), devp<void>(), bb - 1, st), GSDD_E_ARG, false);
        EXPECT(gsdd_mse(devp(), devp(), 1 << 24, 1.f, devp(), devp<void>(), 8192, st), GSDD_OK, true);
        EXPECT(gsdd_mse(devp(), devp(), 1 << 24, 1.f, devp(), devp<void>(), 8191, st), GSDD_E_ARG, false);
        EXPECT(gsdd_axial_attention(devp(), 2, 16, 16, 16, 256, 2, devp(), GSDD_AXIAL_AUTO, st), GSDD_OK, true);
        EXPECT(gsdd_axial_attention(devp(), 2, 16, 16, 16, 256, 2, devp(), GSDD_AXIAL_VALU, st), GSDD_OK, true);
        EXPECT(gsdd_axial_attention(devp(), 2, 16, 16, 16, 256, 2, devp(), 5, st), GSDD_E_ARG, false);
        EXPECT(gsdd_axial_attention_bwd(devp(), devp(), 2, 16, 16, 16, 256, 2, devp(), GSDD_AXIAL_AUTO, st), GSDD_OK, true);
        EXPECT(gsdd_axial_attention_bwd(devp(), devp(), 2, 16, 16, 16, 256, 2, devp(), -2, st), GSDD_E_ARG, false);
        // one rule for both directions, judged before the first launch: lines above 64 KB of LDS run (the attribute is requested for
        // them), S = 64 at d = 128 is refused by both although its W and H axes could have been launched
        for (int variant = GSDD_AXIAL_AUTO; variant <= GSDD_AXIAL_VALU; ++variant) {
            EXPECT(gsdd_axial_attention(devp(), 1, 4, 32, 32, 256, 2, devp(), variant, st), GSDD_OK, true);
            EXPECT(gsdd_axial_attention_bwd(devp(), devp(), 1, 4, 32, 32, 256, 2, devp(), variant, st), GSDD_OK, true);
            EXPECT(gsdd_axial_attention(devp(), 1, 63, 64, 64, 128, 2, devp(), variant, st), GSDD_OK, true);
            EXPECT(gsdd_axial_attention_bwd(devp(), devp(), 1, 63, 64, 64, 128, 2, devp(), variant, st), GSDD_OK, true);
            EXPECT(gsdd_axial_attention(devp(), 1, 63, 1, 1, 256, 2, devp(), variant, st), GSDD_OK, true);
            EXPECT(gsdd_axial_attention_bwd(devp(), devp(), 1, 63, 1, 1, 256, 2, devp(), variant, st), GSDD_OK, true);
            EXPECT(gsdd_axial_attention(devp(), 1, 64, 16, 16, 256, 2, devp(), variant, st), GSDD_E_ARG, false);
            EXPECT(gsdd_axial_attention_bwd(devp(), devp(), 1, 64, 16, 16, 256, 2, devp(), variant, st), GSDD_E_ARG, false);
            EXPECT(gsdd_axial_attention(devp(), 1, 2, 2, 65, 8, 2, devp(), variant, st), GSDD_E_ARG, false);
            EXPECT(gsdd_axial_attention_bwd(devp(), devp(), 1, 2, 2, 65, 8, 2, devp(), variant, st), GSDD_E_ARG, false);
        }
        if (gsdd_axial_attention_lds_bytes(64, 64, 1) != 99328 || gsdd_axial_attention_lds_bytes(32, 128, 0) != 53632 ||
            gsdd_axial_attention_lds_bytes(64, 128, 0) != -1 || gsdd_axial_attention_lds_bytes(0, 8, 0) != -1) {
            std::fprintf(stderr, "FAIL gsdd_axial_attention_lds_bytes\n");
            ++g_failed;
        }
        // the generic GEMM at the decoder's largest shape, both back ends, and the weight gradient
        gsdd_gemm_desc g;
        std::memset(&g, 0, sizeof g);
        g.in = devp(); g.N = 16; g.Di = 19; g.Hi = 66; g.Wi = 66; g.Cin = 256; g.in_pitch = 256;
        g.Do = 16; g.Ho = 64; g.Wo = 64; g.sd = g.sh = g.sw = 1; g.ntaps = 8; g.taps = devp<int>();
        g.w = devp(); g.Cout = 256; g.epi_shift = devp(); g.act = 1;
        g.out = devp(); g.oD = 16; g.oH = 128; g.oW = 128; g.osd = 1; g.osh = 2; g.osw = 2; g.out_pitch = 256;
        EXPECT(gsdd_gemm(&g, st), GSDD_OK, true);
        g.flags = GSDD_GEMM_EXACT_F32;
        EXPECT(gsdd_gemm(&g, st), GSDD_OK, true);
        EXPECT(gsdd_conv_wgrad(&g, devp(), 256, devp(), st), GSDD_OK, true);
        g.flags = 0;
        EXPECT(gsdd_conv_wgrad(&g, devp(), 256, devp(), st), GSDD_OK, true);
        g.flags = 6;
        EXPECT(gsdd_gemm(&g, st), GSDD_E_ARG, false);
        EXPECT(gsdd_conv_wgrad(&g, devp(), 256, devp(), st), GSDD_E_ARG, false);
        g.flags = 0; g.out_pitch = 100;
        EXPECT(gsdd_gemm(&g, st), GSDD_E_ARG, false);
    }

    // ---------------------------------------------------------------- CLIP text tower: the host copies of ids / eot are read HERE
    {
        const int Bt = 64, S = 22, pitch = 77, C = 512, vocab = 49408, heads = 8;
        int64_t* ids = devp<int64_t>();
        int64_t* eot = devp<int64_t>();
        float *tok = devp(), *pos = devp(), *x = devp(), *qkv = devp(), *att = devp(), *pooled = devp();
        std::vector<int64_t> ids_h((size_t)Bt * pitch, 0), eot_h(Bt, S - 1);
        for (int b = 0; b < Bt; ++b) { ids_h[(size_t)b * pitch] = vocab - 2; ids_h[(size_t)b * pitch + S - 1] = vocab - 1; }
        EXPECT(gsdd_text_embed(ids, ids_h.data(), Bt, S, pitch, C, tok, vocab, pos, 77, x, st), GSDD_OK, true);
        EXPECT(gsdd_text_embed(ids, nullptr, Bt, S, pitch, C, tok, vocab, pos, 77, x, st), GSDD_OK, true);
        EXPECT(gsdd_text_embed(ids, ids_h.data(), Bt, 77, pitch, C, tok, vocab, pos, 77, x, st), GSDD_OK, true);   // the last row's last id is read
        ids_h[(size_t)(Bt - 1) * pitch + S - 1] = vocab;
        EXPECT(gsdd_text_embed(ids, ids_h.data(), Bt, S, pitch, C, tok, vocab, pos, 77, x, st), GSDD_E_ARG, false);
        EXPECT(gsdd_text_embed(ids, ids_h.data(), Bt, S - 1, pitch, C, tok, vocab, pos, 77, x, st), GSDD_OK, true);  // behind S: not looked at
        ids_h[(size_t)(Bt - 1) * pitch + S - 1] = -1;
        EXPECT(gsdd_text_embed(ids, ids_h.data(), Bt, S, pitch, C, tok, vocab, pos, 77, x, st), GSDD_E_ARG, false);
        EXPECT(gsdd_text_embed(nullptr, nullptr, Bt, S, pitch, C, tok, vocab, pos, 77, x, st), GSDD_E_ARG, false);
        EXPECT(gsdd_text_embed(ids, nullptr, Bt, S, pitch, C, nullptr, vocab, pos, 77, x, st), GSDD_E_ARG, false);
        EXPECT(gsdd_text_embed(ids, nullptr, Bt, 78, 78, C, tok, vocab, pos, 78, x, st), GSDD_E_ARG, false);
        EXPECT(gsdd_text_embed(ids, nullptr, Bt, S, S - 1, C, tok, vocab, pos, 77, x, st), GSDD_E_ARG, false);
        EXPECT(gsdd_text_embed(ids, nullptr, Bt, S, pitch, C, tok, vocab, pos, S - 1, x, st), GSDD_E_ARG, false);
        EXPECT(gsdd_text_embed(ids, nullptr, Bt, S, pitch, 510, tok, vocab, pos, 77, x, st), GSDD_E_ARG, false);
        EXPECT(gsdd_text_embed(ids, nullptr, 0, S, pitch, C, tok, vocab, pos, 77, x, st), GSDD_E_ARG, false);
        EXPECT(gsdd_text_embed(ids, nullptr, Bt, S, pitch, C, tok + 1, vocab, pos, 77, x, st), GSDD_E_ARG, false);

        for (int s : {1, 16, 17, 77}) EXPECT(gsdd_text_attention(qkv, Bt, s, C, heads, 0.125f, att, st), GSDD_OK, true);
        EXPECT(gsdd_text_attention(qkv, Bt, S, 64, 2, 0.1767767f, att, st), GSDD_OK, true);                  // d = 32
        EXPECT(gsdd_text_attention(qkv, Bt, S, 32, 2, 0.25f, att, st), GSDD_OK, true);                       // d = 16
        EXPECT(gsdd_text_attention(qkv, Bt, 78, C, heads, 0.125f, att, st), GSDD_E_ARG, false);
        EXPECT(gsdd_text_attention(qkv, Bt, 0, C, heads, 0.125f, att, st), GSDD_E_ARG, false);
        EXPECT(gsdd_text_attention(qkv, Bt, S, C, 3, 0.125f, att, st), GSDD_E_ARG, false);
        EXPECT(gsdd_text_attention(qkv, Bt, S, C, 4, 0.125f, att, st), GSDD_E_ARG, false);                   // d = 128
        EXPECT(gsdd_text_attention(qkv, Bt, S, C, 0, 0.125f, att, st), GSDD_E_ARG, false);
        EXPECT(gsdd_text_attention(qkv, Bt, S, C, heads, 0.f, att, st), GSDD_E_ARG, false);
        EXPECT(gsdd_text_attention(nullptr, Bt, S, C, heads, 0.125f, att, st), GSDD_E_ARG, false);
        EXPECT(gsdd_text_attention(qkv, Bt, S, C, heads, 0.125f, nullptr, st), GSDD_E_ARG, false);
        EXPECT(gsdd_text_attention(qkv, 1 << 29, S, C, heads, 0.125f, att, st), GSDD_E_ARG, false);          // grid beyond 2^31

        EXPECT(gsdd_text_pool(x, eot, eot_h.data(), Bt, S, C, pooled, st), GSDD_OK, true);
        EXPECT(gsdd_text_pool(x, eot, nullptr, Bt, S, C, pooled, st), GSDD_OK, true);
        eot_h[Bt - 1] = S;
        EXPECT(gsdd_text_pool(x, eot, eot_h.data(), Bt, S, C, pooled, st), GSDD_E_ARG, false);
        eot_h[Bt - 1] = -1;
        EXPECT(gsdd_text_pool(x, eot, eot_h.data(), Bt, S, C, pooled, st), GSDD_E_ARG, false);
        EXPECT(gsdd_text_pool(x, nullptr, nullptr, Bt, S, C, pooled, st), GSDD_E_ARG, false);
        EXPECT(gsdd_text_pool(nullptr, eot, nullptr, Bt, S, C, pooled, st), GSDD_E_ARG, false);
        EXPECT(gsdd_text_pool(x, eot, nullptr, Bt, 78, C, pooled, st), GSDD_E_ARG, false);
        EXPECT(gsdd_text_pool(x, eot, nullptr, Bt, S, 6, pooled, st), GSDD_E_ARG, false);
    }

    // ---------------------------------------------------------------- CLIP image tower: frame patches, embed, non-causal attention
    {
        const int Bv = 16, Tv = 16, Hh = 128, R = 224, P = 32, C = 768, heads = 12, S = 50, N = Bv * Tv;
        float *clips = devp((size_t)Bv * 3 * Tv * Hh * Hh * 4), *rows = devp((size_t)N * 49 * 3 * P * P * 4), *pe = devp((size_t)N * 49 * C * 4);
        float *cls = devp(), *pos = devp(), *x = devp((size_t)N * S * C * 4), *qkv = devp((size_t)N * S * 3 * C * 4), *att = devp((size_t)N * S * C * 4);
        EXPECT(gsdd_clip_frame_patches(clips, Bv, Tv, Hh, Hh, R, P, rows, st), GSDD_OK, true);
        EXPECT(gsdd_clip_frame_patches(clips, 2, 3, 8, 8, 8, 8, rows, st), GSDD_OK, true);                   // H == R, one patch
        EXPECT(gsdd_clip_frame_patches(clips, 2, 3, 37, 37, 64, 32, rows, st), GSDD_OK, true);
        EXPECT(gsdd_clip_frame_patches(clips, 1, 1, 1, 1, 4096, 4096, rows, st), GSDD_OK, true);             // the largest resolution
        EXPECT(gsdd_clip_frame_patches(clips, Bv, Tv, Hh, Hh + 1, R, P, rows, st), GSDD_E_ARG, false);       // H != W
        EXPECT(gsdd_clip_frame_patches(clips, Bv, Tv, 256, 256, R, P, rows, st), GSDD_E_ARG, false);         // H > R
        EXPECT(gsdd_clip_frame_patches(clips, Bv, Tv, Hh, Hh, R, 48, rows, st), GSDD_E_ARG, false);          // R % P != 0
        EXPECT(gsdd_clip_frame_patches(clips, Bv, Tv, Hh, Hh, 4128, P, rows, st), GSDD_E_ARG, false);        // R > 4096
        EXPECT(gsdd_clip_frame_patches(clips, Bv, Tv, Hh, Hh, R, 0, rows, st), GSDD_E_ARG, false);
        EXPECT(gsdd_clip_frame_patches(clips, 0, Tv, Hh, Hh, R, P, rows, st), GSDD_E_ARG, false);
        EXPECT(gsdd_clip_frame_patches(clips, Bv, -1, Hh, Hh, R, P, rows, st), GSDD_E_ARG, false);
        EXPECT(gsdd_clip_frame_patches(clips, Bv, Tv, 0, 0, R, P, rows, st), GSDD_E_ARG, false);
        EXPECT(gsdd_clip_frame_patches(nullptr, Bv, Tv, Hh, Hh, R, P, rows, st), GSDD_E_ARG, false);
        EXPECT(gsdd_clip_frame_patches(clips, Bv, Tv, Hh, Hh, R, P, nullptr, st), GSDD_E_ARG, false);
        EXPECT(gsdd_clip_frame_patches(clips, 1 << 20, 1 << 10, Hh, Hh, R, P, rows, st), GSDD_E_ARG, false); // grid beyond 2^31
        EXPECT(gsdd_clip_frame_patches(clips, 1 << 30, 1 << 30, 1, 1, 1, 1, rows, st), GSDD_E_ARG, false);   // 2^60 frames

        EXPECT(gsdd_clip_vision_embed(pe, cls, pos, N, S, C, x, st), GSDD_OK, true);
        EXPECT(gsdd_clip_vision_embed(pe, cls, pos, N, 1, C, x, st), GSDD_OK, true);                         // the class token alone
        EXPECT(gsdd_clip_vision_embed(pe, cls, pos, N, 77, C, x, st), GSDD_OK, true);
        EXPECT(gsdd_clip_vision_embed(pe, cls, pos, N, 0, C, x, st), GSDD_E_ARG, false);
        EXPECT(gsdd_clip_vision_embed(pe, cls, pos, N, 78, C, x, st), GSDD_E_ARG, false);
        EXPECT(gsdd_clip_vision_embed(pe, cls, pos, N, S, 766, x, st), GSDD_E_ARG, false);
        EXPECT(gsdd_clip_vision_embed(pe, cls, pos, 0, S, C, x, st), GSDD_E_ARG, false);
        EXPECT(gsdd_clip_vision_embed(nullptr, cls, pos, N, S, C, x, st), GSDD_E_ARG, false);
        EXPECT(gsdd_clip_vision_embed(pe, nullptr, pos, N, S, C, x, st), GSDD_E_ARG, false);
        EXPECT(gsdd_clip_vision_embed(pe, cls, nullptr, N, S, C, x, st), GSDD_E_ARG, false);
        EXPECT(gsdd_clip_vision_embed(pe, cls, pos, N, S, C, nullptr, st), GSDD_E_ARG, false);
        EXPECT(gsdd_clip_vision_embed(pe, cls + 1, pos, N, S, C, x, st), GSDD_E_ARG, false);                 // misaligned
        EXPECT(gsdd_clip_vision_embed(pe, cls, pos, 1 << 30, 77, 1 << 20, x, st), GSDD_E_ARG, false);        // grid beyond 2^31

        for (int s : {1, 16, 17, 50, 77}) EXPECT(gsdd_clip_attention(qkv, N, s, C, heads, 0.125f, att, st), GSDD_OK, true);
        EXPECT(gsdd_clip_attention(qkv, N, S, 64, 2, 0.1767767f, att, st), GSDD_OK, true);                   // d = 32
        EXPECT(gsdd_clip_attention(qkv, N, S, 32, 2, 0.25f, att, st), GSDD_OK, true);                        // d = 16
        EXPECT(gsdd_clip_attention(qkv, N, 78, C, heads, 0.125f, att, st), GSDD_E_ARG, false);
        EXPECT(gsdd_clip_attention(qkv, N, 0, C, heads, 0.125f, att, st), GSDD_E_ARG, false);
        EXPECT(gsdd_clip_attention(qkv, N, S, C, 5, 0.125f, att, st), GSDD_E_ARG, false);
        EXPECT(gsdd_clip_attention(qkv, N, S, C, 6, 0.125f, att, st), GSDD_E_ARG, false);                    // d = 128
        EXPECT(gsdd_clip_attention(qkv, N, S, C, 0, 0.125f, att, st), GSDD_E_ARG, false);
        EXPECT(gsdd_clip_attention(qkv, N, S, C, heads, 0.f, att, st), GSDD_E_ARG, false);
        EXPECT(gsdd_clip_attention(qkv, N, S, C, heads, NAN, att, st), GSDD_E_ARG, false);
        EXPECT(gsdd_clip_attention(qkv, 0, S, C, heads, 0.125f, att, st), GSDD_E_ARG, false);
        EXPECT(gsdd_clip_attention(nullptr, N, S, C, heads, 0.125f, att, st), GSDD_E_ARG, false);
        EXPECT(gsdd_clip_attention(qkv, N, S, C, heads, 0.125f, nullptr, st), GSDD_E_ARG, false);
        EXPECT(gsdd_clip_attention(qkv + 1, N, S, C, heads, 0.125f, att, st), GSDD_E_ARG, false);            // misaligned
        EXPECT(gsdd_clip_attention(qkv, 1 << 28, S, C, heads, 0.125f, att, st), GSDD_E_ARG, false);          // grid beyond 2^31
    }

    // ---------------------------------------------------------------- optimiser stage: norm, finalize, AdamW + EMA, swap
    {
        const int nb = 1122;             // the C4 transformer's parameters in blocks of up to 4096 elements
        int64_t* table = devp<int64_t>((size_t)nb * 7 * 8);
        double* partials = devp<double>((size_t)nb * 8);
        gsdd_optim_state* os = devp<gsdd_optim_state>(sizeof(gsdd_optim_state));
        if (gsdd_abi_sizeof(8) != (int64_t)sizeof(gsdd_optim_state) || gsdd_abi_sizeof(6) != -1) {
            std::fprintf(stderr, "FAIL gsdd_abi_sizeof(8) / (6)\n");
            ++g_failed;
        }
        EXPECT(gsdd_grad_sqnorm(table, nb, partials, st), GSDD_OK, true);
        EXPECT(gsdd_grad_sqnorm(table, 1, partials, st), GSDD_OK, true);
        EXPECT(gsdd_grad_sqnorm(nullptr, nb, partials, st), GSDD_E_ARG, false);
        EXPECT(gsdd_grad_sqnorm(table, nb, nullptr, st), GSDD_E_ARG, false);
        for (int bad : {0, -1}) EXPECT(gsdd_grad_sqnorm(table, bad, partials, st), GSDD_E_ARG, false);
        EXPECT(gsdd_grad_norm_finalize(partials, nb, 1.f, 1, os, st), GSDD_OK, true);
        EXPECT(gsdd_grad_norm_finalize(partials, nb, INFINITY, 0, os, st), GSDD_OK, true);           // no clipping
        EXPECT(gsdd_grad_norm_finalize(nullptr, nb, 1.f, 1, os, st), GSDD_E_ARG, false);
        EXPECT(gsdd_grad_norm_finalize(partials, nb, 1.f, 1, nullptr, st), GSDD_E_ARG, false);
        for (int bad : {0, -1}) EXPECT(gsdd_grad_norm_finalize(partials, bad, 1.f, 1, os, st), GSDD_E_ARG, false);
        for (float bad : {0.f, -1.f, NAN}) EXPECT(gsdd_grad_norm_finalize(partials, nb, bad, 1, os, st), GSDD_E_ARG, false);
        EXPECT(gsdd_adamw_ema_multi(table, nb, 0.9f, 0.96f, 1e-8f, 4.5e-2f, 0.99f, os, st), GSDD_OK, true);
        EXPECT(gsdd_adamw_ema_multi(table, nb, 0.5f, 0.999f, 1e-8f, 0.f, 0.f, os, st), GSDD_OK, true);
        EXPECT(gsdd_adamw_ema_multi(nullptr, nb, 0.9f, 0.96f, 1e-8f, 0.f, 0.f, os, st), GSDD_E_ARG, false);
        EXPECT(gsdd_adamw_ema_multi(table, nb, 0.9f, 0.96f, 1e-8f, 0.f, 0.f, nullptr, st), GSDD_E_ARG, false);
        for (int bad : {0, -1}) EXPECT(gsdd_adamw_ema_multi(table, bad, 0.9f, 0.96f, 1e-8f, 0.f, 0.f, os, st), GSDD_E_ARG, false);
        for (float bad : {-1e-3f, NAN}) EXPECT(gsdd_adamw_ema_multi(table, nb, 0.9f, 0.96f, 1e-8f, bad, 0.f, os, st), GSDD_E_ARG, false);
        for (float bad : {-0.1f, 1.f, 1.5f, NAN}) EXPECT(gsdd_adamw_ema_multi(table, nb, 0.9f, 0.96f, 1e-8f, 0.f, bad, os, st), GSDD_E_ARG, false);
        EXPECT(gsdd_swap_multi(table, nb, st), GSDD_OK, true);
        EXPECT(gsdd_swap_multi(nullptr, nb, st), GSDD_E_ARG, false);
        for (int bad : {0, -1}) EXPECT(gsdd_swap_multi(table, bad, st), GSDD_E_ARG, false);
    }

    // ---------------------------------------------------------------- GIF export: the device entries' checks; median cut and encoder RUN here
    {
        const int Bv = 16, Tv = 16, Hh = 128;
        float* clips = devp((size_t)Bv * 3 * Tv * Hh * Hh * 4);
        uint32_t *hist = devp<uint32_t>((size_t)Bv * Tv * 32768 * 4), *sums = devp<uint32_t>((size_t)Bv * Tv * 1024 * 4);
        uint8_t *box = devp<uint8_t>((size_t)Bv * Tv * 32768), *pal = devp<uint8_t>((size_t)Bv * Tv * 1024), *idx = devp<uint8_t>((size_t)Bv * Tv * Hh * Hh);
        int32_t* ncol = devp<int32_t>((size_t)Bv * Tv * 4);
        for (int pf = 0; pf <= 1; ++pf) {
            EXPECT(gsdd_gif_histogram(clips, Bv, Tv, Hh, Hh, pf, hist, st), GSDD_OK, true);
            EXPECT(gsdd_gif_box_sums(clips, Bv, Tv, Hh, Hh, pf, box, sums, st), GSDD_OK, true);
            for (int d : {0, 1, 64}) EXPECT(gsdd_gif_map(clips, Bv, Tv, Hh, Hh, pf, pal, ncol, d, idx, st), GSDD_OK, true);
        }
        EXPECT(gsdd_gif_histogram(clips, 1, 1, 1, 1, 0, hist, st), GSDD_OK, true);
        EXPECT(gsdd_gif_histogram(clips, 1, 1, 4096, 4096, 1, hist, st), GSDD_OK, true);                     // 2^24 pixels: the largest group
        EXPECT(gsdd_gif_histogram(clips, 1, 2, 4096, 4096, 0, hist, st), GSDD_E_ARG, false);                 // 2^25 pixels in a clip
        EXPECT(gsdd_gif_histogram(clips, 1, 2, 4096, 4096, 1, hist, st), GSDD_OK, true);                     // ... but 2^24 in a frame
        EXPECT(gsdd_gif_histogram(clips, 1, 1, 1, 65535, 0, hist, st), GSDD_OK, true);
        EXPECT(gsdd_gif_histogram(clips, 1, 1, 1, 65536, 0, hist, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_histogram(clips, 1, 1, 65536, 1, 0, hist, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_histogram(clips, 0, Tv, Hh, Hh, 0, hist, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_histogram(clips, Bv, -1, Hh, Hh, 0, hist, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_histogram(clips, Bv, Tv, Hh, Hh, 2, hist, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_histogram(nullptr, Bv, Tv, Hh, Hh, 0, hist, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_histogram(clips, Bv, Tv, Hh, Hh, 0, nullptr, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_histogram(clips, 1 << 30, 4, 1, 1, 1, hist, st), GSDD_E_ARG, false);                 // 2^32 frames
        EXPECT(gsdd_gif_histogram(clips, 1 << 21, 1, 4096, 4096, 0, hist, st), GSDD_E_ARG, false);           // grid of 2^31
        EXPECT(gsdd_gif_box_sums(clips, Bv, Tv, Hh, Hh, 0, nullptr, sums, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_box_sums(clips, Bv, Tv, Hh, Hh, 0, box, nullptr, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_box_sums(clips, Bv, Tv, Hh, Hh, 0, box + 1, sums, st), GSDD_E_ARG, false);           // misaligned table
        EXPECT(gsdd_gif_box_sums(clips, Bv, Tv, 0, Hh, 0, box, sums, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_box_sums(clips, 1, 2, 4096, 4096, 0, box, sums, st), GSDD_E_ARG, false);
        for (int bad : {-1, 65, 1000}) EXPECT(gsdd_gif_map(clips, Bv, Tv, Hh, Hh, 0, pal, ncol, bad, idx, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_map(clips, Bv, Tv, Hh, Hh, 0, nullptr, ncol, 0, idx, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_map(clips, Bv, Tv, Hh, Hh, 0, pal, nullptr, 0, idx, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_map(clips, Bv, Tv, Hh, Hh, 0, pal, ncol, 0, nullptr, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_map(clips, Bv, Tv, Hh, Hh, 0, pal + 2, ncol, 0, idx, st), GSDD_E_ARG, false);        // misaligned palette
        EXPECT(gsdd_gif_map(clips, Bv, Tv, Hh, 70000, 0, pal, ncol, 0, idx, st), GSDD_E_ARG, false);
        // palette refinement and error diffusion (csrc/gif_refine.hip)
        uint64_t* sse = devp<uint64_t>((size_t)Bv * Tv * 8);
        for (int pf = 0; pf <= 1; ++pf) {
            EXPECT(gsdd_gif_palette_sums(clips, Bv, Tv, Hh, Hh, pf, pal, ncol, sums, sse, st), GSDD_OK, true);
            EXPECT(gsdd_gif_diffuse(clips, Bv, Tv, Hh, Hh, pf, pal, ncol, idx, st), GSDD_OK, true);
        }
        EXPECT(gsdd_gif_diffuse(clips, 1, 1, 1, 65535, 0, pal, ncol, idx, st), GSDD_OK, true);                // one row, the widest
        EXPECT(gsdd_gif_diffuse(clips, 1, 1, 65535, 1, 0, pal, ncol, idx, st), GSDD_OK, true);                // 64 bands of one column
        EXPECT(gsdd_gif_diffuse(clips, 1, 1, 1025, 16368, 0, pal, ncol, idx, st), GSDD_OK, true);             // the longest band row
        EXPECT(gsdd_gif_diffuse(clips, 1, 1, 1025, 16369, 0, pal, ncol, idx, st), GSDD_E_ARG, false);         // more than 2^24 pixels
        EXPECT(gsdd_gif_palette_sums(clips, 1, 2, 4096, 4096, 0, pal, ncol, sums, sse, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_palette_sums(nullptr, Bv, Tv, Hh, Hh, 0, pal, ncol, sums, sse, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_palette_sums(clips, Bv, Tv, Hh, Hh, 0, nullptr, ncol, sums, sse, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_palette_sums(clips, Bv, Tv, Hh, Hh, 0, pal, nullptr, sums, sse, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_palette_sums(clips, Bv, Tv, Hh, Hh, 0, pal, ncol, nullptr, sse, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_palette_sums(clips, Bv, Tv, Hh, Hh, 0, pal, ncol, sums, nullptr, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_palette_sums(clips, Bv, Tv, Hh, Hh, 0, pal + 2, ncol, sums, sse, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_palette_sums(clips, Bv, Tv, Hh, Hh, 0, pal, ncol, sums, (uint64_t*)((uint8_t*)sse + 4), st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_diffuse(nullptr, Bv, Tv, Hh, Hh, 0, pal, ncol, idx, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_diffuse(clips, Bv, Tv, Hh, Hh, 0, nullptr, ncol, idx, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_diffuse(clips, Bv, Tv, Hh, Hh, 0, pal, nullptr, idx, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_diffuse(clips, Bv, Tv, Hh, Hh, 0, pal, ncol, nullptr, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_diffuse(clips, Bv, Tv, Hh, Hh, 0, pal + 1, ncol, idx, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_diffuse(clips, Bv, Tv, Hh, Hh, 2, pal, ncol, idx, st), GSDD_E_ARG, false);

        // median cut on real host memory: a smooth ramp, every bin, one bin, nothing
        std::vector<uint32_t> h(32768, 0u);
        std::vector<uint8_t> bx(32768, 7);
        int nb = -1;
        for (int i = 0; i < 32768; ++i) h[i] = (uint32_t)((i * 2654435761u) >> 28);
        for (int colors : {2, 16, 255, 256}) {
            EXPECT(gsdd_gif_median_cut(h.data(), colors, bx.data(), &nb), GSDD_OK, false);
            if (nb != colors) { std::fprintf(stderr, "FAIL median cut made %d boxes of %d\n", nb, colors); ++g_failed; }
        }
        std::fill(h.begin(), h.end(), 0xFFFFFFFFu);                                                          // 2^47 pixels: 64-bit counts
        EXPECT(gsdd_gif_median_cut(h.data(), 256, bx.data(), &nb), GSDD_OK, false);
        std::fill(h.begin(), h.end(), 0u);
        EXPECT(gsdd_gif_median_cut(h.data(), 256, bx.data(), &nb), GSDD_OK, false);
        if (nb != 0 || bx[0] != 255) { std::fprintf(stderr, "FAIL median cut of an empty histogram\n"); ++g_failed; }
        h[32767] = 5u;
        EXPECT(gsdd_gif_median_cut(h.data(), 2, bx.data(), &nb), GSDD_OK, false);
        if (nb != 1 || bx[32767] != 0) { std::fprintf(stderr, "FAIL median cut of one bin\n"); ++g_failed; }
        for (int bad : {-1, 0, 1, 257}) EXPECT(gsdd_gif_median_cut(h.data(), bad, bx.data(), &nb), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_median_cut(nullptr, 16, bx.data(), &nb), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_median_cut(h.data(), 16, nullptr, &nb), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_median_cut(h.data(), 16, bx.data(), nullptr), GSDD_E_ARG, false);

        // encoder: exact-size heap buffers, so that one byte too many is a sanitizer report
        const int Te = 3, He = 96, We = 96;
        std::vector<uint8_t> px((size_t)Te * He * We), table((size_t)Te * 768);
        for (size_t i = 0; i < table.size(); ++i) table[i] = (uint8_t)(i * 7);
        uint32_t lcg = 1u;
        auto fill = [&](int n) { for (auto& v : px) { lcg = lcg * 1664525u + 1013904223u; v = (uint8_t)((lcg >> 24) % (uint32_t)n); } };
        auto encode_exact = [&](const int32_t* nc, int npal, int T2) -> int64_t {
            std::vector<uint8_t> big((size_t)gsdd_gif_encode_bound(T2, He, We));
            int64_t clears = -1;
            const int64_t n = gsdd_gif_encode(px.data(), T2, He, We, table.data(), nc, npal, 20, 0, big.data(), (int64_t)big.size(), &clears);
            ++g_checked;
            if (n <= 0 || clears < T2) { std::fprintf(stderr, "FAIL gsdd_gif_encode -> %lld [%s]\n", (long long)n, gsdd_last_error()); ++g_failed; return n; }
            std::vector<uint8_t> exact((size_t)n), shorter((size_t)n - 1);
            ++g_checked;
            if (gsdd_gif_encode(px.data(), T2, He, We, table.data(), nc, npal, 20, 0, exact.data(), n, nullptr) != n ||
                std::memcmp(exact.data(), big.data(), (size_t)n) != 0) { std::fprintf(stderr, "FAIL gsdd_gif_encode at the exact size\n"); ++g_failed; }
            ++g_checked;
            if (gsdd_gif_encode(px.data(), T2, He, We, table.data(), nc, npal, 20, 0, shorter.data(), n - 1, nullptr) != GSDD_E_CAP) {
                std::fprintf(stderr, "FAIL gsdd_gif_encode one byte short\n"); ++g_failed; }
            ++g_checked;
            if (gsdd_gif_encode(px.data(), T2, He, We, table.data(), nc, npal, 20, 0, shorter.data(), 0, nullptr) != GSDD_E_CAP) {
                std::fprintf(stderr, "FAIL gsdd_gif_encode into nothing\n"); ++g_failed; }
            return n;
        };
        const int32_t one_colour[1] = {1}, full[1] = {256}, mixed[3] = {2, 5, 256};
        fill(1);
        encode_exact(one_colour, 1, Te);                                                                     // a 1-colour table
        fill(256);
        encode_exact(full, 1, Te);                                                                           // 256 colours: mid-stream clears
        encode_exact(full, 1, 1);
        fill(2);
        encode_exact(mixed, 3, Te);                                                                          // local tables
        std::vector<uint8_t> out((size_t)gsdd_gif_encode_bound(Te, He, We));
        const int64_t cap = (int64_t)out.size();
        fill(256);
        EXPECT((int)gsdd_gif_encode(px.data(), Te, He, We, table.data(), mixed, 3, 20, 0, out.data(), cap, nullptr), GSDD_E_ARG, false);  // index >= n_colors
        const int32_t zero[1] = {0}, many[1] = {257};
        EXPECT((int)gsdd_gif_encode(px.data(), Te, He, We, table.data(), zero, 1, 20, 0, out.data(), cap, nullptr), GSDD_E_ARG, false);
        EXPECT((int)gsdd_gif_encode(px.data(), Te, He, We, table.data(), many, 1, 20, 0, out.data(), cap, nullptr), GSDD_E_ARG, false);
        EXPECT((int)gsdd_gif_encode(px.data(), Te, He, We, table.data(), mixed, 2, 20, 0, out.data(), cap, nullptr), GSDD_E_ARG, false);   // 2 palettes, 3 frames
        EXPECT((int)gsdd_gif_encode(px.data(), Te, He, We, table.data(), full, 1, -1, 0, out.data(), cap, nullptr), GSDD_E_ARG, false);
        EXPECT((int)gsdd_gif_encode(px.data(), Te, He, We, table.data(), full, 1, 20, 65536, out.data(), cap, nullptr), GSDD_E_ARG, false);
        EXPECT((int)gsdd_gif_encode(px.data(), 0, He, We, table.data(), full, 1, 20, 0, out.data(), cap, nullptr), GSDD_E_ARG, false);
        EXPECT((int)gsdd_gif_encode(px.data(), Te, He, We, table.data(), full, 1, 20, 0, out.data(), -1, nullptr), GSDD_E_ARG, false);
        EXPECT((int)gsdd_gif_encode(nullptr, Te, He, We, table.data(), full, 1, 20, 0, out.data(), cap, nullptr), GSDD_E_ARG, false);
        EXPECT((int)gsdd_gif_encode(px.data(), Te, He, We, nullptr, full, 1, 20, 0, out.data(), cap, nullptr), GSDD_E_ARG, false);
        EXPECT((int)gsdd_gif_encode(px.data(), Te, He, We, table.data(), nullptr, 1, 20, 0, out.data(), cap, nullptr), GSDD_E_ARG, false);
        EXPECT((int)gsdd_gif_encode(px.data(), Te, He, We, table.data(), full, 1, 20, 0, nullptr, cap, nullptr), GSDD_E_ARG, false);
        EXPECT((int)gsdd_gif_encode_bound(0, He, We), GSDD_E_ARG, false);
        EXPECT((int)gsdd_gif_encode_bound(1, 65536, We), GSDD_E_ARG, false);

        // the delta stage (csrc/gif_delta.hip): the device entry's checks ...
        {
            int32_t* rects = devp<int32_t>((size_t)Bv * Tv * 16);
            uint32_t* changed = devp<uint32_t>((size_t)Bv * Tv * 4);
            uint8_t* dout = devp<uint8_t>((size_t)Bv * Tv * Hh * Hh);
            for (int pf = 0; pf <= 1; ++pf)
                for (int tol : {0, 1, 195075}) EXPECT(gsdd_gif_delta(clips, idx, Bv, Tv, Hh, Hh, pf, pal, ncol, tol, dout, rects, changed, st), GSDD_OK, true);
            EXPECT(gsdd_gif_delta(clips, idx, 1, 300, 5, 3, 0, pal, ncol, 0, dout, rects, changed, st), GSDD_OK, true);
            EXPECT(gsdd_gif_delta(clips, idx, 1, 1, 4096, 4096, 1, pal, ncol, 48, dout, rects, changed, st), GSDD_OK, true);    // 2^24 pixels
            EXPECT(gsdd_gif_delta(clips, idx, 1, 2, 4096, 4096, 0, pal, ncol, 0, dout, rects, changed, st), GSDD_E_ARG, false);
            EXPECT(gsdd_gif_delta(clips, idx, 1, 1, 1, 65536, 0, pal, ncol, 0, dout, rects, changed, st), GSDD_E_ARG, false);
            EXPECT(gsdd_gif_delta(clips, idx, 0, Tv, Hh, Hh, 0, pal, ncol, 0, dout, rects, changed, st), GSDD_E_ARG, false);
            EXPECT(gsdd_gif_delta(clips, idx, Bv, Tv, Hh, Hh, 2, pal, ncol, 0, dout, rects, changed, st), GSDD_E_ARG, false);
            for (int bad : {-1, 195076}) EXPECT(gsdd_gif_delta(clips, idx, Bv, Tv, Hh, Hh, 0, pal, ncol, bad, dout, rects, changed, st), GSDD_E_ARG, false);
            EXPECT(gsdd_gif_delta(nullptr, idx, Bv, Tv, Hh, Hh, 0, pal, ncol, 0, dout, rects, changed, st), GSDD_E_ARG, false);
            EXPECT(gsdd_gif_delta(clips, nullptr, Bv, Tv, Hh, Hh, 0, pal, ncol, 0, dout, rects, changed, st), GSDD_E_ARG, false);
            EXPECT(gsdd_gif_delta(clips, idx, Bv, Tv, Hh, Hh, 0, nullptr, ncol, 0, dout, rects, changed, st), GSDD_E_ARG, false);
            EXPECT(gsdd_gif_delta(clips, idx, Bv, Tv, Hh, Hh, 0, pal, nullptr, 0, dout, rects, changed, st), GSDD_E_ARG, false);
            EXPECT(gsdd_gif_delta(clips, idx, Bv, Tv, Hh, Hh, 0, pal, ncol, 0, nullptr, rects, changed, st), GSDD_E_ARG, false);
            EXPECT(gsdd_gif_delta(clips, idx, Bv, Tv, Hh, Hh, 0, pal, ncol, 0, dout, nullptr, changed, st), GSDD_E_ARG, false);
            EXPECT(gsdd_gif_delta(clips, idx, Bv, Tv, Hh, Hh, 0, pal, ncol, 0, dout, rects, nullptr, st), GSDD_E_ARG, false);
            EXPECT(gsdd_gif_delta(clips, idx, Bv, Tv, Hh, Hh, 0, pal + 2, ncol, 0, dout, rects, changed, st), GSDD_E_ARG, false);
            EXPECT(gsdd_gif_delta(clips, idx, Bv, Tv, Hh, Hh, 0, pal, ncol, 0, idx, rects, changed, st), GSDD_E_ARG, false);       // out is indices
        }
        // paired video metrics (csrc/paired_metrics.hip): every form pairing launches once; the checks return before a launch
        {
            int32_t* parts = devp<int32_t>();
            const uint8_t* bytes = idx;                                                                          // a uint8 operand: any alignment
            for (int fa = 0; fa <= 1; ++fa)
                for (int fb = 0; fb <= 1; ++fb)
                    for (int ssim = 0; ssim <= 1; ++ssim)
                        EXPECT(gsdd_paired_metrics(fa ? (const void*)(bytes + 1) : (const void*)clips, fa, fb ? (const void*)bytes : (const void*)clips, fb,
                                                   Bv, Tv, Hh, Hh, ssim, parts, st), GSDD_OK, true);
            EXPECT(gsdd_paired_metrics(clips, 0, bytes, 1, 1, 1, 11, 11, 1, parts, st), GSDD_OK, true);         // one window
            EXPECT(gsdd_paired_metrics(clips, 0, bytes, 1, 1, 1, 1, 1, 0, parts, st), GSDD_OK, true);           // the squared error alone: any plane
            EXPECT(gsdd_paired_metrics(clips, 0, bytes, 1, 2, 3, 5, 3, 0, parts, st), GSDD_OK, true);
            EXPECT(gsdd_paired_metrics(clips, 0, bytes, 1, 1, 1, 46340, 46340, 0, parts, st), GSDD_OK, true);   // just below 2^31 pixels
            EXPECT((int)gsdd_paired_metrics_tiles(128, 128), 64, false);
            EXPECT((int)gsdd_paired_metrics_tiles(10, 3), 1, false);
            EXPECT((int)gsdd_paired_metrics_tiles(0, 3), GSDD_E_ARG, false);
            EXPECT((int)gsdd_paired_metrics_tiles(3, -1), GSDD_E_ARG, false);
            EXPECT(gsdd_paired_metrics(clips, 0, bytes, 1, 1, 1, 10, 16, 1, parts, st), GSDD_E_ARG, false);     // SSIM needs 11 x 11
            EXPECT(gsdd_paired_metrics(clips, 0, bytes, 1, 1, 1, 16, 10, 1, parts, st), GSDD_E_ARG, false);
            for (int bad : {-1, 2}) {
                EXPECT(gsdd_paired_metrics(clips, bad, bytes, 1, Bv, Tv, Hh, Hh, 1, parts, st), GSDD_E_ARG, false);
                EXPECT(gsdd_paired_metrics(clips, 0, bytes, bad, Bv, Tv, Hh, Hh, 1, parts, st), GSDD_E_ARG, false);
                EXPECT(gsdd_paired_metrics(clips, 0, bytes, 1, Bv, Tv, Hh, Hh, bad, parts, st), GSDD_E_ARG, false);
            }
            EXPECT(gsdd_paired_metrics(clips, 0, bytes, 1, 0, Tv, Hh, Hh, 1, parts, st), GSDD_E_ARG, false);
            EXPECT(gsdd_paired_metrics(clips, 0, bytes, 1, Bv, -1, Hh, Hh, 1, parts, st), GSDD_E_ARG, false);
            EXPECT(gsdd_paired_metrics(clips, 0, bytes, 1, Bv, Tv, 0, Hh, 0, parts, st), GSDD_E_ARG, false);
            EXPECT(gsdd_paired_metrics(clips, 0, bytes, 1, Bv, Tv, Hh, 0, 0, parts, st), GSDD_E_ARG, false);
            EXPECT(gsdd_paired_metrics(clips, 0, bytes, 1, 1, 1, 65536, 32768, 0, parts, st), GSDD_E_ARG, false);      // 2^31 pixels in a plane
            EXPECT(gsdd_paired_metrics(clips, 0, bytes, 1, 1 << 30, 3, Hh, Hh, 0, parts, st), GSDD_E_ARG, false);      // 9 * 2^30 planes
            EXPECT(gsdd_paired_metrics(clips, 0, bytes, 1, 1 << 16, 1 << 8, 128, 128, 1, parts, st), GSDD_E_ARG, false);   // 2^31 workgroups and more
            EXPECT(gsdd_paired_metrics(nullptr, 0, bytes, 1, Bv, Tv, Hh, Hh, 1, parts, st), GSDD_E_ARG, false);
            EXPECT(gsdd_paired_metrics(clips, 0, nullptr, 1, Bv, Tv, Hh, Hh, 1, parts, st), GSDD_E_ARG, false);
            EXPECT(gsdd_paired_metrics(clips, 0, bytes, 1, Bv, Tv, Hh, Hh, 1, nullptr, st), GSDD_E_ARG, false);
            EXPECT(gsdd_paired_metrics(bytes + 2, 0, bytes, 1, Bv, Tv, Hh, Hh, 1, parts, st), GSDD_E_ARG, false);     // a float operand off its alignment
            EXPECT(gsdd_paired_metrics(clips, 0, bytes + 1, 0, Bv, Tv, Hh, Hh, 1, parts, st), GSDD_E_ARG, false);
            EXPECT(gsdd_paired_metrics(clips, 0, bytes, 1, Bv, Tv, Hh, Hh, 1, (int32_t*)(bytes + 2), st), GSDD_E_ARG, false);
        }
        // LPIPS (csrc/lpips.hip): the stem operand in both forms and the distance head at every tap width; the checks return before a launch
        {
            const uint8_t* bytes = idx;
            const float* table = devp();
            float *rows = devp(), *feat = devp(), *w = devp();
            double* parts = devp<double>();
            const int64_t frames = (int64_t)Bv * Tv;
            for (int form = 0; form <= 1; ++form)
                for (int padw : {0, 1, 2, 64})
                    EXPECT(gsdd_lpips_stem_rows(form ? (const void*)(bytes + 1) : (const void*)clips, form, Bv, Tv, Hh, Hh, 0, frames, padw, table, rows, st),
                           GSDD_OK, true);
            EXPECT(gsdd_lpips_stem_rows(clips, 0, Bv, Tv, 1, 1, frames - 1, 1, 0, table, rows, st), GSDD_OK, true);          // the last frame alone
            EXPECT(gsdd_lpips_stem_rows(clips, 0, 1, 1, 46340, 46340, 0, 1, 2, table, rows, st), GSDD_OK, true);             // just below 2^31 pixels
            for (int bad : {-1, 2}) EXPECT(gsdd_lpips_stem_rows(clips, bad, Bv, Tv, Hh, Hh, 0, frames, 2, table, rows, st), GSDD_E_ARG, false);
            for (int bad : {-1, 65}) EXPECT(gsdd_lpips_stem_rows(clips, 0, Bv, Tv, Hh, Hh, 0, frames, bad, table, rows, st), GSDD_E_ARG, false);
            EXPECT(gsdd_lpips_stem_rows(clips, 0, 0, Tv, Hh, Hh, 0, 1, 2, table, rows, st), GSDD_E_ARG, false);
            EXPECT(gsdd_lpips_stem_rows(clips, 0, Bv, -1, Hh, Hh, 0, 1, 2, table, rows, st), GSDD_E_ARG, false);
            EXPECT(gsdd_lpips_stem_rows(clips, 0, Bv, Tv, 0, Hh, 0, 1, 2, table, rows, st), GSDD_E_ARG, false);
            EXPECT(gsdd_lpips_stem_rows(clips, 0, Bv, Tv, Hh, 0, 0, 1, 2, table, rows, st), GSDD_E_ARG, false);
            EXPECT(gsdd_lpips_stem_rows(clips, 0, Bv, Tv, Hh, Hh, -1, 1, 2, table, rows, st), GSDD_E_ARG, false);            // frames outside the clips
            EXPECT(gsdd_lpips_stem_rows(clips, 0, Bv, Tv, Hh, Hh, 0, 0, 2, table, rows, st), GSDD_E_ARG, false);
            EXPECT(gsdd_lpips_stem_rows(clips, 0, Bv, Tv, Hh, Hh, 1, frames, 2, table, rows, st), GSDD_E_ARG, false);
            EXPECT(gsdd_lpips_stem_rows(clips, 0, Bv, Tv, Hh, Hh, frames, 1, 2, table, rows, st), GSDD_E_ARG, false);
            EXPECT(gsdd_lpips_stem_rows(clips, 0, Bv, Tv, Hh, Hh, 0, INT64_MAX, 2, table, rows, st), GSDD_E_ARG, false);
            EXPECT(gsdd_lpips_stem_rows(clips, 0, 1, 1, 65536, 32768, 0, 1, 2, table, rows, st), GSDD_E_ARG, false);         // 2^31 pixels in a frame
            EXPECT(gsdd_lpips_stem_rows(clips, 0, 1 << 16, 1 << 15, Hh, Hh, 0, 1, 2, table, rows, st), GSDD_E_ARG, false);   // 2^31 frames
            EXPECT(gsdd_lpips_stem_rows(clips, 0, 1 << 15, 1 << 15, 2048, 2048, 0, 1 << 29, 2, table, rows, st), GSDD_E_ARG, false);   // too many workgroups
            EXPECT(gsdd_lpips_stem_rows(nullptr, 0, Bv, Tv, Hh, Hh, 0, frames, 2, table, rows, st), GSDD_E_ARG, false);
            EXPECT(gsdd_lpips_stem_rows(clips, 0, Bv, Tv, Hh, Hh, 0, frames, 2, nullptr, rows, st), GSDD_E_ARG, false);
            EXPECT(gsdd_lpips_stem_rows(clips, 0, Bv, Tv, Hh, Hh, 0, frames, 2, table, nullptr, st), GSDD_E_ARG, false);
            EXPECT(gsdd_lpips_stem_rows(bytes + 2, 0, Bv, Tv, Hh, Hh, 0, frames, 2, table, rows, st), GSDD_E_ARG, false);    // a float operand off its alignment
            EXPECT(gsdd_lpips_stem_rows(clips, 0, Bv, Tv, Hh, Hh, 0, frames, 2, (const float*)(bytes + 1), rows, st), GSDD_E_ARG, false);
            EXPECT(gsdd_lpips_stem_rows(clips, 0, Bv, Tv, Hh, Hh, 0, frames, 2, table, rows + 1, st), GSDD_E_ARG, false);    // out needs 16 bytes
            for (int C : {4, 64, 128, 192, 256, 384, 512})
                for (int64_t P : {(int64_t)1, (int64_t)961, (int64_t)16384})
                    EXPECT(gsdd_lpips_layer_distance(feat, w, frames, P, C, parts, st), GSDD_OK, true);
            EXPECT((int)gsdd_lpips_distance_slots(961, 64), 8, false);
            EXPECT((int)gsdd_lpips_distance_slots(33, 512), 2, false);
            EXPECT((int)gsdd_lpips_distance_slots(2048, 4), 1, false);
            EXPECT((int)gsdd_lpips_distance_slots(0, 64), GSDD_E_ARG, false);
            EXPECT((int)gsdd_lpips_distance_slots(5, 6), GSDD_E_ARG, false);
            EXPECT((int)gsdd_lpips_distance_slots(5, 516), GSDD_E_ARG, false);
            for (int bad : {0, -4, 2, 6, 516, 1024}) EXPECT(gsdd_lpips_layer_distance(feat, w, frames, 961, bad, parts, st), GSDD_E_ARG, false);
            EXPECT(gsdd_lpips_layer_distance(feat, w, 0, 961, 64, parts, st), GSDD_E_ARG, false);
            EXPECT(gsdd_lpips_layer_distance(feat, w, frames, 0, 64, parts, st), GSDD_E_ARG, false);
            EXPECT(gsdd_lpips_layer_distance(feat, w, 1 << 15, 1 << 15, 64, parts, st), GSDD_E_ARG, false);                 // 2^31 rows
            EXPECT(gsdd_lpips_layer_distance(feat, w, (int64_t)1 << 40, 1, 64, parts, st), GSDD_E_ARG, false);
            EXPECT(gsdd_lpips_layer_distance(feat, w, 1, (int64_t)1 << 40, 64, parts, st), GSDD_E_ARG, false);
            EXPECT(gsdd_lpips_layer_distance(nullptr, w, frames, 961, 64, parts, st), GSDD_E_ARG, false);
            EXPECT(gsdd_lpips_layer_distance(feat, nullptr, frames, 961, 64, parts, st), GSDD_E_ARG, false);
            EXPECT(gsdd_lpips_layer_distance(feat, w, frames, 961, 64, nullptr, st), GSDD_E_ARG, false);
            EXPECT(gsdd_lpips_layer_distance(feat + 1, w, frames, 961, 64, parts, st), GSDD_E_ARG, false);                  // rows are read as float4s
            EXPECT(gsdd_lpips_layer_distance(feat, w + 2, frames, 961, 64, parts, st), GSDD_E_ARG, false);
            EXPECT(gsdd_lpips_layer_distance(feat, w, frames, 961, 64, (double*)(rows + 1), st), GSDD_E_ARG, false);
        }
        // long clips: the slide between two windows and the window blend -- the accepted forms launch, every refusal returns before one
        {
            alignas(16) static unsigned char raw[64];
            int64_t* i64p = (int64_t*)raw;
            uint8_t* u8p = raw;
            int* i32p = (int*)raw;
            float* f32p = (float*)raw;
            const int Bs = 8, F = 16, hw = 256, k = 4, n = 40, Kc = 4096;
            EXPECT(gsdd_d3pm_window_slide(i64p, i64p, i64p, u8p, i64p, i64p, i32p, Bs, F, hw, k, n, Kc, 99, 2 * Bs, 0, st), GSDD_OK, true);
            EXPECT(gsdd_d3pm_window_slide(i64p, i64p, nullptr, nullptr, nullptr, i64p, nullptr, Bs, F, hw, k, n, Kc, 99, 0, 1, st), GSDD_OK, true);
            EXPECT(gsdd_d3pm_window_slide(i64p, i64p, i64p, u8p, i64p, i64p, i32p, 1, 2, 1, 1, 2, 1, 0, 0, 0, st), GSDD_OK, true);     // the smallest
            EXPECT(gsdd_d3pm_window_slide(nullptr, i64p, i64p, u8p, i64p, i64p, i32p, Bs, F, hw, k, n, Kc, 99, 2 * Bs, 0, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_window_slide(i64p, nullptr, i64p, u8p, i64p, i64p, i32p, Bs, F, hw, k, n, Kc, 99, 2 * Bs, 0, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_window_slide(i64p, i64p, nullptr, u8p, i64p, i64p, i32p, Bs, F, hw, k, n, Kc, 99, 2 * Bs, 0, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_window_slide(i64p, i64p, i64p, nullptr, i64p, i64p, i32p, Bs, F, hw, k, n, Kc, 99, 2 * Bs, 0, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_window_slide(i64p, i64p, i64p, u8p, nullptr, i64p, i32p, Bs, F, hw, k, n, Kc, 99, 2 * Bs, 0, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_window_slide(i64p, i64p, i64p, u8p, i64p, nullptr, i32p, Bs, F, hw, k, n, Kc, 99, 2 * Bs, 0, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_window_slide(i64p, i64p, i64p, u8p, i64p, i64p, nullptr, Bs, F, hw, k, n, Kc, 99, 2 * Bs, 0, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_window_slide(i64p, nullptr, nullptr, nullptr, nullptr, i64p, nullptr, Bs, F, hw, k, n, Kc, 99, 0, 1, st), GSDD_E_ARG, false);
            for (int bad : {0, -1, F, F + 1}) EXPECT(gsdd_d3pm_window_slide(i64p, i64p, i64p, u8p, i64p, i64p, i32p, Bs, F, hw, bad, n, Kc, 99, 2 * Bs, 0, st), GSDD_E_ARG, false);      // k >= F
            for (int bad : {F - 1, 0, -40}) EXPECT(gsdd_d3pm_window_slide(i64p, i64p, i64p, u8p, i64p, i64p, i32p, Bs, F, hw, k, bad, Kc, 99, 2 * Bs, 0, st), GSDD_E_ARG, false);       // n < F
            EXPECT(gsdd_d3pm_window_slide(i64p, i64p, i64p, u8p, i64p, i64p, i32p, 0, F, hw, k, n, Kc, 99, 0, 0, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_window_slide(i64p, i64p, i64p, u8p, i64p, i64p, i32p, -Bs, F, hw, k, n, Kc, 99, 0, 0, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_window_slide(i64p, i64p, i64p, u8p, i64p, i64p, i32p, Bs, -F, hw, k, n, Kc, 99, 0, 0, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_window_slide(i64p, i64p, i64p, u8p, i64p, i64p, i32p, Bs, F, 0, k, n, Kc, 99, 0, 0, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_window_slide(i64p, i64p, i64p, u8p, i64p, i64p, i32p, Bs, F, -hw, k, n, Kc, 99, 0, 0, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_window_slide(i64p, i64p, i64p, u8p, i64p, i64p, i32p, Bs, F, hw, k, n, 0, 99, 0, 0, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_window_slide(i64p, i64p, i64p, u8p, i64p, i64p, i32p, Bs, F, hw, k, n, Kc, -1, 0, 0, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_window_slide(i64p, i64p, i64p, u8p, i64p, i64p, i32p, Bs, F, hw, k, n, Kc, 99, -1, 0, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_window_slide(i64p, i64p, i64p, u8p, i64p, i64p, i32p, Bs, F, hw, k, n, Kc, 99, Bs * F * hw + 1, 0, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_window_slide(i64p, i64p, i64p, u8p, i64p, i64p, i32p, Bs, F, hw, k, n, Kc, 99, 0, 2, st), GSDD_E_ARG, false);
            EXPECT(gsdd_d3pm_window_slide(i64p, i64p, i64p, u8p, i64p, i64p, i32p, 1 << 15, 1 << 8, 1 << 8, k, 1 << 9, Kc, 99, 0, 0, st), GSDD_E_ARG, false);   // 2^31 tokens
            const int BC = 48, Fw = 16, HW = 128 * 128, Fo = 40;
            for (int mode : {GSDD_BLEND_LINEAR, GSDD_BLEND_KEEP, GSDD_BLEND_REPLACE}) {
                EXPECT(gsdd_clip_window_blend(f32p, f32p, BC, Fw, HW, Fo, 12, 4, mode, st), GSDD_OK, true);
                EXPECT(gsdd_clip_window_blend(f32p, f32p, BC, Fw, HW, Fo, 0, 0, mode, st), GSDD_OK, true);
                EXPECT(gsdd_clip_window_blend(f32p, f32p, BC, Fw, 35, Fo, 36, 4, mode, st), GSDD_OK, mode != GSDD_BLEND_KEEP);     // only the overlap fits: keep writes nothing
            }
            EXPECT(gsdd_clip_window_blend(nullptr, f32p, BC, Fw, HW, Fo, 12, 4, 0, st), GSDD_E_ARG, false);
            EXPECT(gsdd_clip_window_blend(f32p, nullptr, BC, Fw, HW, Fo, 12, 4, 0, st), GSDD_E_ARG, false);
            for (int bad : {Fw, Fw + 1, -1}) EXPECT(gsdd_clip_window_blend(f32p, f32p, BC, Fw, HW, Fo, 12, bad, 0, st), GSDD_E_ARG, false);     // k >= F
            for (int bad : {Fw - 1, 0, -Fo}) EXPECT(gsdd_clip_window_blend(f32p, f32p, BC, Fw, HW, bad, 0, 0, 0, st), GSDD_E_ARG, false);       // n < F
            for (int bad : {0, -3, 65536}) EXPECT(gsdd_clip_window_blend(f32p, f32p, bad, Fw, HW, Fo, 12, 4, 0, st), GSDD_E_ARG, false);
            for (int bad : {0, -16}) EXPECT(gsdd_clip_window_blend(f32p, f32p, BC, bad, HW, Fo, 12, 0, 0, st), GSDD_E_ARG, false);
            for (int bad : {0, -35}) EXPECT(gsdd_clip_window_blend(f32p, f32p, BC, Fw, bad, Fo, 12, 4, 0, st), GSDD_E_ARG, false);
            for (int bad : {-1, Fo, Fo + 7}) EXPECT(gsdd_clip_window_blend(f32p, f32p, BC, Fw, HW, Fo, bad, 0, 0, st), GSDD_E_ARG, false);
            EXPECT(gsdd_clip_window_blend(f32p, f32p, BC, Fw, HW, Fo, 0, 4, 0, st), GSDD_E_ARG, false);                    // an overlapped first window
            for (int bad : {-1, 3}) EXPECT(gsdd_clip_window_blend(f32p, f32p, BC, Fw, HW, Fo, 12, 4, bad, st), GSDD_E_ARG, false);
            EXPECT(gsdd_clip_window_blend(f32p, f32p, BC, 1 << 12, 1 << 19, 1 << 12, 0, 0, 0, st), GSDD_E_ARG, false);      // 2^31 floats in a window
            EXPECT(gsdd_clip_window_blend((const float*)(raw + 2), f32p, BC, Fw, HW, Fo, 12, 4, 0, st), GSDD_E_ARG, false);
            EXPECT(gsdd_clip_window_blend(f32p, (float*)(raw + 1), BC, Fw, HW, Fo, 12, 4, 0, st), GSDD_E_ARG, false);
        }
        // ... and its encoder, which RUNS here: two frames of 7 x 5 in a buffer of exactly T H W bytes (a row read past a rectangle or past
        // the last frame is a report), frame 1 with the empty marker and then with a one-pixel rectangle in the last corner
        {
            const int Td = 2, Hd = 5, Wd = 7;
            std::vector<uint8_t> dpx((size_t)Td * Hd * Wd);
            for (size_t i = 0; i < dpx.size(); ++i) dpx[i] = (uint8_t)(i % 3);
            for (size_t i = (size_t)Hd * Wd; i < dpx.size(); ++i) dpx[i] = 3;                                    // frame 1: all transparent
            const int32_t nc3[1] = {3}, tr3[1] = {3}, none[1] = {-1}, nc2[2] = {3, 3}, tr2[2] = {-1, 3};
            int32_t boxes[8] = {0, 0, Wd - 1, Hd - 1, Wd, Hd, -1, -1};
            std::vector<uint8_t> dbig((size_t)gsdd_gif_encode_bound(Td, Hd, Wd));
            auto delta_exact = [&](const int32_t* nc, const int32_t* tr, int npal) {
                int64_t clears = -1;
                const int64_t n = gsdd_gif_encode_delta(dpx.data(), Td, Hd, Wd, table.data(), nc, npal, boxes, tr, 20, 0, dbig.data(), (int64_t)dbig.size(), &clears);
                ++g_checked;
                if (n <= 0 || clears != Td) { std::fprintf(stderr, "FAIL gsdd_gif_encode_delta -> %lld [%s]\n", (long long)n, gsdd_last_error()); ++g_failed; return; }
                std::vector<uint8_t> exact((size_t)n), shorter((size_t)n - 1);
                ++g_checked;
                if (gsdd_gif_encode_delta(dpx.data(), Td, Hd, Wd, table.data(), nc, npal, boxes, tr, 20, 0, exact.data(), n, nullptr) != n ||
                    std::memcmp(exact.data(), dbig.data(), (size_t)n) != 0) { std::fprintf(stderr, "FAIL gsdd_gif_encode_delta at the exact size\n"); ++g_failed; }
                ++g_checked;
                if (gsdd_gif_encode_delta(dpx.data(), Td, Hd, Wd, table.data(), nc, npal, boxes, tr, 20, 0, shorter.data(), n - 1, nullptr) != GSDD_E_CAP) {
                    std::fprintf(stderr, "FAIL gsdd_gif_encode_delta one byte short\n"); ++g_failed; }
                // what it wrote is a GIF the library's own decoder takes: two frames, frame 1 with the rectangle asked for
                int64_t info[8] = {0};
                ++g_checked;
                if (gsdd_gif_probe(exact.data(), n, info) != GSDD_OK || info[0] != Wd || info[1] != Hd || info[2] != Td) {
                    std::fprintf(stderr, "FAIL gsdd_gif_probe of the delta file [%s]\n", gsdd_last_error()); ++g_failed; }
            };
            dpx[(size_t)Hd * Wd] = 0;                                                                           // the pixel the 1 x 1 image of an empty frame shows
            delta_exact(nc3, tr3, 1);                                                                            // the empty marker, a global table
            delta_exact(nc2, tr2, 2);                                                                            // local tables, one without a transparent index
            boxes[4] = Wd - 1, boxes[5] = Hd - 1, boxes[6] = Wd - 1, boxes[7] = Hd - 1;                          // one pixel, the canvas's last
            dpx.back() = 1;
            delta_exact(nc3, tr3, 1);
            delta_exact(nc3, none, 1);                                                                           // (every index 3 is outside the rectangle: not read)
            const int64_t dcap = (int64_t)dbig.size();
            auto bad_box = [&](int x0, int y0, int x1, int y1) {
                const int32_t b[8] = {0, 0, Wd - 1, Hd - 1, x0, y0, x1, y1};
                EXPECT((int)gsdd_gif_encode_delta(dpx.data(), Td, Hd, Wd, table.data(), nc3, 1, b, tr3, 20, 0, dbig.data(), dcap, nullptr), GSDD_E_ARG, false);
            };
            bad_box(0, 0, Wd, 0);                                                                                // leaves the canvas
            bad_box(0, 0, 0, Hd);
            bad_box(-1, 0, 2, 2);
            bad_box(3, 0, 2, 2);                                                                                 // inverted
            bad_box(0, 3, 2, 2);
            bad_box(Wd, Hd, -1, 0);                                                                              // half an empty marker
            const int32_t tr_hi[1] = {256}, tr_lo[1] = {-2}, nc1[1] = {1}, tr255[1] = {255}, zero[1] = {0}, many[1] = {257};
            EXPECT((int)gsdd_gif_encode_delta(dpx.data(), Td, Hd, Wd, table.data(), nc3, 1, boxes, tr_hi, 20, 0, dbig.data(), dcap, nullptr), GSDD_E_ARG, false);
            EXPECT((int)gsdd_gif_encode_delta(dpx.data(), Td, Hd, Wd, table.data(), nc3, 1, boxes, tr_lo, 20, 0, dbig.data(), dcap, nullptr), GSDD_E_ARG, false);
            EXPECT((int)gsdd_gif_encode_delta(dpx.data(), Td, Hd, Wd, table.data(), nc1, 1, boxes, tr255, 20, 0, dbig.data(), dcap, nullptr), GSDD_E_ARG, false);  // index beyond its table
            EXPECT((int)gsdd_gif_encode_delta(dpx.data(), Td, Hd, Wd, table.data(), zero, 1, boxes, tr3, 20, 0, dbig.data(), dcap, nullptr), GSDD_E_ARG, false);
            EXPECT((int)gsdd_gif_encode_delta(dpx.data(), Td, Hd, Wd, table.data(), many, 1, boxes, tr3, 20, 0, dbig.data(), dcap, nullptr), GSDD_E_ARG, false);
            EXPECT((int)gsdd_gif_encode_delta(dpx.data(), 3, Hd, Wd, table.data(), nc2, 2, boxes, tr2, 20, 0, dbig.data(), dcap, nullptr), GSDD_E_ARG, false);    // 2 palettes, 3 frames
            EXPECT((int)gsdd_gif_encode_delta(dpx.data(), Td, Hd, Wd, table.data(), nc3, 1, boxes, tr3, -1, 0, dbig.data(), dcap, nullptr), GSDD_E_ARG, false);
            EXPECT((int)gsdd_gif_encode_delta(dpx.data(), Td, Hd, Wd, table.data(), nc3, 1, boxes, tr3, 20, 65536, dbig.data(), dcap, nullptr), GSDD_E_ARG, false);
            EXPECT((int)gsdd_gif_encode_delta(dpx.data(), 0, Hd, Wd, table.data(), nc3, 1, boxes, tr3, 20, 0, dbig.data(), dcap, nullptr), GSDD_E_ARG, false);
            EXPECT((int)gsdd_gif_encode_delta(dpx.data(), Td, Hd, 65536, table.data(), nc3, 1, boxes, tr3, 20, 0, dbig.data(), dcap, nullptr), GSDD_E_ARG, false);
            EXPECT((int)gsdd_gif_encode_delta(dpx.data(), Td, Hd, Wd, table.data(), nc3, 1, boxes, tr3, 20, 0, dbig.data(), -1, nullptr), GSDD_E_ARG, false);
            EXPECT((int)gsdd_gif_encode_delta(nullptr, Td, Hd, Wd, table.data(), nc3, 1, boxes, tr3, 20, 0, dbig.data(), dcap, nullptr), GSDD_E_ARG, false);
            EXPECT((int)gsdd_gif_encode_delta(dpx.data(), Td, Hd, Wd, nullptr, nc3, 1, boxes, tr3, 20, 0, dbig.data(), dcap, nullptr), GSDD_E_ARG, false);
            EXPECT((int)gsdd_gif_encode_delta(dpx.data(), Td, Hd, Wd, table.data(), nullptr, 1, boxes, tr3, 20, 0, dbig.data(), dcap, nullptr), GSDD_E_ARG, false);
            EXPECT((int)gsdd_gif_encode_delta(dpx.data(), Td, Hd, Wd, table.data(), nc3, 1, nullptr, tr3, 20, 0, dbig.data(), dcap, nullptr), GSDD_E_ARG, false);
            EXPECT((int)gsdd_gif_encode_delta(dpx.data(), Td, Hd, Wd, table.data(), nc3, 1, boxes, nullptr, 20, 0, dbig.data(), dcap, nullptr), GSDD_E_ARG, false);
            EXPECT((int)gsdd_gif_encode_delta(dpx.data(), Td, Hd, Wd, table.data(), nc3, 1, boxes, tr3, 20, 0, nullptr, dcap, nullptr), GSDD_E_ARG, false);
        }
    }

    // ---------------------------------------------------------------- GIF import: the decoder of FOREIGN bytes RUNS here, on exact-size heap copies
    {
        // probe, then decode into exact-size tables, then once more with the raster one byte short; -> the decode's (or the failed probe's) code
        auto walk_file = [&](const std::vector<uint8_t>& file, std::vector<uint8_t>* raster_out = nullptr) -> int {
            const int64_t n = (int64_t)file.size();
            uint8_t* d = new uint8_t[(size_t)n];                                                             // (n = 0: a valid pointer to nothing)
            std::copy(file.begin(), file.end(), d);
            int64_t info[8];
            int rc = gsdd_gif_probe(d, n, info);
            ++g_checked;
            if (rc != GSDD_OK && rc != GSDD_E_ARG) { std::fprintf(stderr, "FAIL gsdd_gif_probe -> %d\n", rc); ++g_failed; }
            if (rc == GSDD_OK) {
                const size_t F = (size_t)info[2], P = (size_t)info[3], total = (size_t)info[4];
                std::vector<int32_t> frames(F * 8), delays(F);
                std::vector<uint8_t> palettes(P * 1024), raster(total), shorter(total - 1);
                rc = gsdd_gif_decode(d, n, frames.data(), delays.data(), palettes.data(), raster.data(), (int64_t)total);
                ++g_checked;
                if (rc != GSDD_OK && rc != GSDD_E_ARG) { std::fprintf(stderr, "FAIL gsdd_gif_decode -> %d\n", rc); ++g_failed; }
                if (rc == GSDD_OK) {
                    uint8_t* nothing = new uint8_t[0];
                    const int rc_short = gsdd_gif_decode(d, n, frames.data(), delays.data(), palettes.data(),
                                                         total > 1 ? shorter.data() : nothing, (int64_t)total - 1);
                    delete[] nothing;
                    ++g_checked;
                    if (rc_short != GSDD_E_CAP) { std::fprintf(stderr, "FAIL gsdd_gif_decode one raster byte short -> %d\n", rc_short); ++g_failed; }
                    if (raster_out) *raster_out = raster;
                }
            }
            delete[] d;
            return rc;
        };
        auto expect_file = [&](const char* what, const std::vector<uint8_t>& file, int want) {
            const int rc = walk_file(file);
            ++g_checked;
            if (rc != want) { std::fprintf(stderr, "FAIL GIF import of %s -> %d (want %d) [%s]\n", what, rc, want, gsdd_last_error()); ++g_failed; }
        };
        // the project's own writer's files: 96 x 96 noise with mid-stream clear codes, global and local tables
        {
            const int Te = 2, He = 96, We = 96;
            std::vector<uint8_t> px((size_t)Te * He * We), table((size_t)Te * 768);
            uint32_t lcg = 7u;
            for (auto& v : px) { lcg = lcg * 1664525u + 1013904223u; v = (uint8_t)(lcg >> 24); }
            for (size_t i = 0; i < table.size(); ++i) table[i] = (uint8_t)(i * 5);
            const int32_t full[2] = {256, 256};
            for (int npal : {1, 2}) {
                std::vector<uint8_t> file((size_t)gsdd_gif_encode_bound(Te, He, We)), raster;
                const int64_t n = gsdd_gif_encode(px.data(), Te, He, We, table.data(), full, npal, 20, 0, file.data(), (int64_t)file.size(), nullptr);
                file.resize((size_t)(n > 0 ? n : 0));
                const int rc = walk_file(file, &raster);
                ++g_checked;
                if (rc != GSDD_OK || raster != px) { std::fprintf(stderr, "FAIL the writer's file does not decode to its pixels (%d)\n", rc); ++g_failed; }
            }
        }
        // a hand-made file: 3-bit codes with a clear code before every pair of pixels, so that the width never changes
        auto stream = [](const std::vector<int>& codes) {
            std::vector<uint8_t> bytes;
            uint32_t acc = 0;
            int nbits = 0;
            for (int c : codes) { acc |= (uint32_t)c << nbits; nbits += 3; while (nbits >= 8) { bytes.push_back((uint8_t)acc); acc >>= 8; nbits -= 8; } }
            if (nbits) bytes.push_back((uint8_t)acc);
            std::vector<uint8_t> out;
            out.push_back(2);                                                                                // minimum code size
            for (size_t i = 0; i < bytes.size(); i += 2) {                                                   // sub-blocks of 2 bytes
                const size_t len = std::min<size_t>(2, bytes.size() - i);
                out.push_back((uint8_t)len);
                out.insert(out.end(), bytes.begin() + (long)i, bytes.begin() + (long)(i + len));
            }
            out.push_back(0);
            return out;
        };
        auto image = [&](int x, int y, int w, int h, int flags, const std::vector<int>& codes) {
            std::vector<uint8_t> out = {0x2C, (uint8_t)x, 0, (uint8_t)y, 0, (uint8_t)w, 0, (uint8_t)h, 0, (uint8_t)flags};
            const std::vector<uint8_t> s = stream(codes);
            out.insert(out.end(), s.begin(), s.end());
            return out;
        };
        auto cat = [](std::vector<uint8_t> a, const std::vector<uint8_t>& b) { a.insert(a.end(), b.begin(), b.end()); return a; };
        const std::vector<uint8_t> head = {'G', 'I', 'F', '8', '9', 'a', 4, 0, 3, 0, 0x81, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
        const std::vector<uint8_t> loop = {0x21, 0xFF, 11, 'N', 'E', 'T', 'S', 'C', 'A', 'P', 'E', '2', '.', '0', 3, 1, 5, 0, 0};
        const std::vector<uint8_t> gce = {0x21, 0xF9, 4, 0x09, 7, 0, 2, 0}, trailer = {0x3B};
        const std::vector<int> twelve = {4, 0, 1, 4, 2, 3, 4, 0, 6, 4, 1, 2, 4, 3, 3, 4, 0, 0, 5};               // 2 + 2 + 3 (KwKwK) + 2 + 2 + 2 pixels: one too many
        std::vector<uint8_t> good = cat(cat(cat(head, loop), image(0, 0, 4, 3, 0, twelve)), gce);
        good = cat(cat(good, image(1, 0, 2, 3, 0x40, {4, 1, 1, 4, 2, 2, 4, 3, 3, 5})), trailer);                // interlaced 2 x 3
        {
            std::vector<uint8_t> raster;
            const int rc = walk_file(good, &raster);
            const std::vector<uint8_t> want = {0, 1, 2, 3, 0, 0, 0, 1, 2, 3, 3, 0, /* rows 0, 2, 1 of the stored 1 1 | 2 2 | 3 3 */ 1, 1, 3, 3, 2, 2};
            ++g_checked;
            if (rc != GSDD_OK || raster != want) { std::fprintf(stderr, "FAIL the hand-made GIF (%d) [%s]\n", rc, gsdd_last_error()); ++g_failed; }
        }
        int accepted = 0;
        for (size_t n = 0; n < good.size(); ++n) {                                                           // every truncation
            const int rc = walk_file(std::vector<uint8_t>(good.begin(), good.begin() + (long)n));
            accepted += rc == GSDD_OK;
        }
        ++g_checked;
        if (accepted != 3) { std::fprintf(stderr, "FAIL %d truncations of the hand-made GIF decode (want 3: behind frame 0, behind frame 1's control extension, behind frame 1)\n", accepted); ++g_failed; }
        const std::vector<uint8_t> body = cat(head, {});
        auto patched = [&](size_t at, uint8_t v) { std::vector<uint8_t> f = cat(cat(head, image(0, 0, 4, 3, 0, twelve)), trailer); f[at] = v; return f; };
        expect_file("a good single frame", patched(0, 'G'), GSDD_OK);
        expect_file("a bad signature", patched(3, '9'), GSDD_E_ARG);
        expect_file("an empty canvas", patched(6, 0), GSDD_E_ARG);
        expect_file("x + w beyond the canvas", patched(head.size() + 1, 1), GSDD_E_ARG);
        expect_file("y + h beyond the canvas", patched(head.size() + 3, 1), GSDD_E_ARG);
        expect_file("w = 0", patched(head.size() + 5, 0), GSDD_E_ARG);
        expect_file("h = 0", patched(head.size() + 7, 0), GSDD_E_ARG);
        expect_file("minimum code size 0", patched(head.size() + 10, 0), GSDD_E_ARG);
        expect_file("minimum code size 9", patched(head.size() + 10, 9), GSDD_E_ARG);
        expect_file("an unknown block", patched(head.size(), 0x2D), GSDD_E_ARG);
        expect_file("a table without its flag", patched(10, 0x01), GSDD_E_ARG);
        expect_file("no frames, a trailer", cat(body, trailer), GSDD_E_ARG);
        expect_file("no frames, no trailer", body, GSDD_E_ARG);
        expect_file("no frames, extensions only", cat(cat(cat(body, loop), gce), trailer), GSDD_E_ARG);
        expect_file("a code above the next free entry", cat(cat(head, image(0, 0, 4, 3, 0, {4, 0, 7, 5})), trailer), GSDD_E_ARG);
        expect_file("a first code that is no literal", cat(cat(head, image(0, 0, 4, 3, 0, {4, 6, 5})), trailer), GSDD_E_ARG);
        expect_file("the same behind a second clear code", cat(cat(head, image(0, 0, 4, 3, 0, {4, 0, 4, 7, 5})), trailer), GSDD_E_ARG);
        expect_file("an end code before w * h pixels", cat(cat(head, image(0, 0, 4, 3, 0, {4, 0, 1, 5})), trailer), GSDD_E_ARG);
        expect_file("a chain that closes before w * h pixels", cat(cat(head, image(0, 0, 4, 3, 0, {4, 0, 1})), trailer), GSDD_E_ARG);
        expect_file("pixels beyond w * h", cat(cat(head, image(0, 0, 1, 1, 0, twelve)), trailer), GSDD_OK);
        {
            std::vector<uint8_t> cut = cat(head, image(0, 0, 4, 3, 0, twelve));
            cut.pop_back();                                                                                  // the chain's zero length
            expect_file("a chain without its end", cut, GSDD_E_ARG);
            cut.pop_back();
            expect_file("a chain cut inside a sub-block", cut, GSDD_E_ARG);
        }
        int64_t info[8];
        int32_t fr[8], dl[1];
        uint8_t pl[1024], rs[16];
        EXPECT(gsdd_gif_probe(nullptr, 10, info), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_probe(good.data(), (int64_t)good.size(), nullptr), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_probe(good.data(), -1, info), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_decode(nullptr, 10, fr, dl, pl, rs, 16), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_decode(good.data(), (int64_t)good.size(), nullptr, dl, pl, rs, 16), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_decode(good.data(), (int64_t)good.size(), fr, nullptr, pl, rs, 16), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_decode(good.data(), (int64_t)good.size(), fr, dl, nullptr, rs, 16), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_decode(good.data(), (int64_t)good.size(), fr, dl, pl, nullptr, 16), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_decode(good.data(), (int64_t)good.size(), fr, dl, pl, rs, -1), GSDD_E_ARG, false);

        // the compositor's checks (fake device pointers; select_host is real host memory, exact size)
        const int F = 16, W = 128, H = 128;
        uint8_t *raster = devp<uint8_t>((size_t)F * W * H), *pal = devp<uint8_t>(1024), *out = devp<uint8_t>((size_t)F * W * H * 3);
        int32_t *frames = devp<int32_t>((size_t)F * 32), *sel = devp<int32_t>((size_t)F * 4);
        std::vector<int32_t> all(F), padded = {0, 4, 8, 15, 15, 15}, one = {15}, down = {0, 2, 1}, below = {-1, 0}, above = {0, 16};
        for (int i = 0; i < F; ++i) all[i] = i;
        EXPECT(gsdd_gif_compose(raster, frames, pal, F, W, H, sel, all.data(), F, 0, out, st), GSDD_OK, true);
        EXPECT(gsdd_gif_compose(raster, frames, pal, F, W, H, sel, padded.data(), 6, 0xFFFFFF, out, st), GSDD_OK, true);
        EXPECT(gsdd_gif_compose(raster, frames, pal, F, W, H, sel, one.data(), 1, 0x102030, out, st), GSDD_OK, true);
        EXPECT(gsdd_gif_compose(raster, frames, pal, F, 1, 1, sel, one.data(), 1, 0, out, st), GSDD_OK, true);
        EXPECT(gsdd_gif_compose(raster, frames, pal, F, 65535, 65535, sel, one.data(), 1, 0, out, st), GSDD_OK, true);   // 2^32 - 131071 pixels
        EXPECT(gsdd_gif_compose(raster, frames, pal, F, W, H, sel, down.data(), 3, 0, out, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_compose(raster, frames, pal, F, W, H, sel, below.data(), 2, 0, out, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_compose(raster, frames, pal, F, W, H, sel, above.data(), 2, 0, out, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_compose(raster, frames, pal, F, W, H, sel, all.data(), 0, 0, out, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_compose(raster, frames, pal, F, W, H, sel, all.data(), -1, 0, out, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_compose(raster, frames, pal, 0, W, H, sel, all.data(), 1, 0, out, st), GSDD_E_ARG, false);
        for (int bad : {0, -1, 65536}) {
            EXPECT(gsdd_gif_compose(raster, frames, pal, F, bad, H, sel, all.data(), F, 0, out, st), GSDD_E_ARG, false);
            EXPECT(gsdd_gif_compose(raster, frames, pal, F, W, bad, sel, all.data(), F, 0, out, st), GSDD_E_ARG, false);
        }
        for (int bad : {-1, 1 << 24}) EXPECT(gsdd_gif_compose(raster, frames, pal, F, W, H, sel, all.data(), F, bad, out, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_compose(nullptr, frames, pal, F, W, H, sel, all.data(), F, 0, out, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_compose(raster, nullptr, pal, F, W, H, sel, all.data(), F, 0, out, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_compose(raster, frames, nullptr, F, W, H, sel, all.data(), F, 0, out, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_compose(raster, frames, pal, F, W, H, nullptr, all.data(), F, 0, out, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_compose(raster, frames, pal, F, W, H, sel, nullptr, F, 0, out, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_compose(raster, frames, pal, F, W, H, sel, all.data(), F, 0, nullptr, st), GSDD_E_ARG, false);
        EXPECT(gsdd_gif_compose(raster, frames, pal + 2, F, W, H, sel, all.data(), F, 0, out, st), GSDD_E_ARG, false);   // misaligned palette
    }

    // ---------------------------------------------------------------- graph capture misuse, events
    {
        void* exec = nullptr;
        EXPECT(gsdd_graph_end(st, &exec), GSDD_E_HIP, false);                         // end without begin
        EXPECT(gsdd_graph_begin(st), GSDD_OK, false);
        EXPECT(gsdd_graph_begin(st), GSDD_E_HIP, false);                              // nested begin
        EXPECT(gsdd_graph_end(st, &exec), GSDD_OK, false);
        EXPECT(gsdd_graph_launch(exec, st), GSDD_OK, false);
        EXPECT(gsdd_graph_launch(nullptr, st), GSDD_E_ARG, false);
        EXPECT(gsdd_graph_destroy(exec), GSDD_OK, false);
        EXPECT(gsdd_graph_end(st, nullptr), GSDD_E_ARG, false);
        void *e0 = nullptr, *e1 = nullptr;
        float ms = -1.f;
        EXPECT(gsdd_event_create(&e0), GSDD_OK, false);
        EXPECT(gsdd_event_create(&e1), GSDD_OK, false);
        EXPECT(gsdd_event_record(e0, st), GSDD_OK, false);
        EXPECT(gsdd_event_elapsed_ms(e0, e1, &ms), GSDD_OK, false);
        EXPECT(gsdd_event_elapsed_ms(e0, nullptr, &ms), GSDD_E_ARG, false);
        EXPECT(gsdd_event_destroy(e0), GSDD_OK, false);
        EXPECT(gsdd_event_destroy(e1), GSDD_OK, false);
        EXPECT(gsdd_event_create(nullptr), GSDD_E_ARG, false);
    }

    std::printf("host_asan driver: %d expectations, %d failed, %ld launches validated\n", g_checked, g_failed, gsdd_stub_launches());
    return g_failed == 0 ? 0 : 1;
}
