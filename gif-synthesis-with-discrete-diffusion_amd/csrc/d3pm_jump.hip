// Forward jump of a D3PM state: x_b ~ q(x_b | x_a), b = a + jump, per position and independently (RePaint's resampling, the move
// back up the chain between two passes over the same levels).
//
// The mask-and-uniform chain composes in closed form: from level a to level b a [MASK] stays [MASK]; a code i becomes [MASK] with
// probability gamma~, stays i with alpha~ + beta~ and becomes any other code with beta~ each, where alpha~ = abar_b / abar_a,
// 1 - gamma~ = (1 - gbar_b) / (1 - gbar_a), beta~ = (1 - alpha~ - gamma~) / K.  The three logarithms come from a host-made fp64 table
// (beta~ is a difference of numbers of size 1e-5 at the top of the schedule: not formed in f32 here), indexed by the from-level
// wrapped modulo T + 1 (level -1, clean, is index T).
//
// One wave64 owns one position, four positions per workgroup, as in the reverse step; the draw is the step's draw of a known position
// (known_row_draw, d3pm_rows.hpp): Gumbel arg-max over the K + 1 classes on the position's own counters of one (B, K + 1, L) Philox
// stream, first index on ties.  No row lives in registers and nothing but the token, three floats and the hold byte is read.
#include "common.hpp"
#include "d3pm_rows.hpp"

namespace gsdd {

template <int J, bool FULL>
__global__ __launch_bounds__(256) void d3pm_forward_jump_kernel(gsdd_jump_desc d) {
    const int lane = threadIdx.x & 63;
    const int64_t pos = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (pos >= (int64_t)d.B * d.L) return;
    const int K = d.K;
    const int tok = __builtin_amdgcn_readfirstlane((int)d.tok_in[pos]);
    int win = tok;
    // wave-uniform shortcuts: a held position and a [MASK] (absorbing) are copied through and read no uniforms
    const bool held = d.hold != nullptr && __builtin_amdgcn_readfirstlane((int)d.hold[pos]) != 0;
    if (!held && tok != K) {
        const int b = (int)(pos / d.L);
        const int64_t T1 = (int64_t)d.T + 1;
        const int64_t a = ((d.t_dev[b] % T1) + T1) % T1;           // the from-level, -1 = T: always a row of the table
        const float* row = d.table + 3 * a;
        win = known_row_draw<J, FULL>(tok, row[0], row[1], row[2], lane, K, d.seed, (uint32_t)d.stream_dev[0], (uint64_t)(d.row0 + pos));
    }
    if (lane == 0) d.tok_out[pos] = win;
}

}  // namespace gsdd

using namespace gsdd;

extern "C" int gsdd_d3pm_forward_jump(const gsdd_jump_desc* d, void* stream) {
    GSDD_CHECK_ARG(d != nullptr, "null descriptor");
    GSDD_CHECK_ARG(d->tok_in && d->tok_out && d->t_dev && d->stream_dev, "null pointer");
    GSDD_CHECK_ARG(d->table != nullptr, "null table (the host-made [(T + 1) * 3] log-probabilities of this jump)");
    GSDD_CHECK_ARG(d->B > 0 && d->L > 0 && d->T > 0, "bad sizes");
    GSDD_CHECK_ARG(d->K >= 4 && d->K % 4 == 0 && d->K <= 8192, "K must be a multiple of 4 in [4, 8192]");
    GSDD_CHECK_ARG(d->jump >= 1, "jump must be >= 1");
    GSDD_CHECK_ARG(d->jump <= d->T, "jump must be <= T (level -1 to level T - 1)");
    const int64_t npos = (int64_t)d->B * d->L;
    const dim3 grid((unsigned)((npos + 3) / 4)), block(256);
    hipStream_t st = (hipStream_t)stream;
    // FULL at K = 4096 only, as the step's families with known positions
    if (d->K == 4096) hipLaunchKernelGGL((d3pm_forward_jump_kernel<16, true>), grid, block, 0, st, *d);
    else for_class_width(d->K, [&](auto jc) {
        constexpr int J = decltype(jc)::value;
        hipLaunchKernelGGL((d3pm_forward_jump_kernel<J, false>), grid, block, 0, st, *d);
    });
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}
