"""The kernels of csrc/d3pm_step.hip -- the training objective (d3pm_train_loss_kernel + d3pm_train_finalize_kernel), its hand-derived
gradient (d3pm_train_bwd_kernel, plain and fused LOSS variant), the reverse step and q_sample -- element by element against a
reference, at every register-grid width J = ceil(K / 256) the API accepts and at position counts B L that are no multiple of the four
positions of a workgroup.

REFERENCE OF THE OBJECTIVE (`forward` + `tail` below, run in fp64 on the device; `dlogits` = torch.autograd.grad(loss, logits) of it).
Written from the formulas of the kernel's header comment and of oracle/d3pm.py:train_loss / q_posterior, not from the oracle's fp32
functions: log-softmax; append -70 and clamp to [-70, 0]; q_posterior of the model row and of the one-hot truth; KL, NLL, auxiliary KL;
the t = 0 switch; / pt; the adaptive weight; / (B L); the Lt_history / Lt_count updates in sample order.  It takes the kernel's own
inputs as exact: the eight f32 schedule buffers cast to double, LOG_ZERO = f32(log 1e-30), pt, mask_weight and aux_weight as their f32
values, and the finalize kernel's literals 0.1f / 0.9f.  torch.clamp's backward passes the gradient on the closed interval, as the
kernel's gates `v >= -70 && v <= 0` do.

BARS, per output element.  U = 2^-24; gamma(k) = U (8 + 2 sqrt(k)) for an f32 sum of k terms (as in test_gpu_gemm_family);
c = 1.7e-7 + U: exp_term(d) = v_exp_f32(d log2 e) has the documented relative error 1.7e-7 |d| (+ 2 U), and d itself is an f32
difference (U |d|).  |.| and all weights below are of the exact (fp64) values; every e_* is an absolute error.
  * a = log_softmax(x): the row sum of exp_term terms is fp64, so lse = max + log(sum) carries e_lse = sum_k p_k (c |x_k - max| + 2 U) + 2 U
    (p = softmax), and a_k, rounded to f32, e_a = e_lse + U |a_k|.  r = clamp(a) inherits e_a.
  * lae(u, v) = max + log(1 + exp(-|u - v|)) in f32: the exponential's argument carries U |u - v| and exp_le0 2 ulp: together at most
    (U |d| + 4 U) e^-|d| <= 1.5 U; the sum 1 + . one rounding (2 U), log_norm (v_log_f32 and a hi/lo product) 2 ulp of a value <= ln 2,
    the final add U |lae|: e_lae = U |lae| + 8 U on top of the propagated input errors (|d lae / du| = sigmoid(u - v) <= 1).
    The four transition constants (qt / q1, hit / miss) are such values of exact inputs with one more f32 add (LOG_ZERO + log_cumprod_at):
    e_const = 2 U |const| + 8 U; for a [MASK] position they are schedule entries, exact.
  * q_k = r_k - lqt_k: e_q = e_a + e_const + U |q_k| (truth row: lx0 is exact, e_q = e_const + U |q_k|; q_K = LOG_ZERO exact).
    S = max + logf(sum_k exp_term(q_k - max)) over K + 1 classes in f32:
    e_S = sum_k pi_k (e_q,k + c |q_k - max| + 2 U) + gamma(K + 1) + 4 U + U |S|,  pi = softmax(q).
  * pre_k = lae(qn_k + alpha, beta) + lq1_k + S with qn = q - S, rho_k = d lae / d qn = exp(qn + alpha - lae) in [0, 1].  S enters with
    weight (1 - rho) <= 1:  e_pre = rho (e_q + U |qn| + U |qn + alpha|) + e_S + U |lae| + 8 U + e_const(lq1) + U |lae + lq1| + U |pre|.
    lm = clamp(pre), ltr likewise: same bars.  probs = exp_le0(lm): probs (e_pre + 2 U).
  * per position: kl = mw sum_k e^ltr (ltr - lm): each term e^ltr ((e_ltr + 2 U) |ltr - lm| + e_ltr + e_lm + U |ltr - lm|) + U |term|, the
    sum gamma(K + 1) sum |term|, the product with mw U |kl|.  nll = -sum w0 lm: sum w0 (e_lm + 6 U |lm|) + gamma(K + 1) sum |w0 lm| + U |nll|
    (w0 = expf(LOG_ZERO) off the truth: 4 U).  aux = mw sum_{k<K} w0 (lx0 - r): sum (w0 (e_a + U |lx0 - r|) + 5 U |term|) + gamma(K) sum |term|.
  * finalize: the three per-sample sums add gamma(L) sum_l |v_l| to the sum of the positions' bars; kl_loss is one of them (the t = 0
    switch multiplies by exact 0 / 1); vb = kl_loss / pt + w aux_weight kl_aux_loss / pt: 2 U and 6 U relative on the two terms + U |vb|;
    loss = sum_b vb / (B L): sum of the vb bars + gamma(B) sum |vb| / (B L) + 3 U |loss|.  acc / keep rate: the count is exact up to
    the positions whose arg-max is undecided (below): n_undecided / L + 2 U.  Lt_history[t] <- 0.1f kl_loss^2 + 0.9f Lt_history[t]:
    0.1 (2 |kl_loss| e + e^2 + U kl_loss^2) + 0.9 e_prev + 3 U |new|, carried along the sample order for a repeated t; Lt_count and
    the entries of timesteps that are not in the batch: bit for bit.
  * dlogits.  With the per-position weights g_kl, g_nll, g_aux (products and one division of exact inputs: 8 U relative =: eg):
      G_k = -(g_kl e^ltr_k + g_nll w0_k):          e_G   = |G| (eg + 5 U) + g_kl e^ltr e_ltr
      Gqn_k = gate(pre_k) G_k rho_k:               e_Gqn = |G| rho e_logrho + rho e_G + U |Gqn|,
          e_logrho = (1 - rho) (e_q + e_S + U |qn| + U |qn + alpha|) + U |lae| + 8 U + U |qn + alpha - lae| + 2 U
      GS = sum_k gate G_k - sum_k Gqn_k:           e_GS  = sum e_G + sum e_Gqn + gamma(K + 1) (sum |G| + sum |Gqn|) + U |GS|
      Gr_k = Gqn_k + GS pi_k - g_aux w0_k:         e_Gr  = e_Gqn + |GS| pi (e_q + e_S + U |qn| + 2 U) + pi e_GS + U |GS pi| + U |Gqn + GS pi|
                                                           + g_aux w0 (eg + 4 U) + U |Gr|
      Ga_k = gate(a_k) Gr_k, sumGa = sum_k Ga_k:   e_sumGa = sum e_Ga + gamma(K) sum |Ga|
      dx_k = Ga_k - p_k sumGa, p_k = exp_term(a_k): e_p = p (c |a| + e_a + 2 U) + 2^-126 (a result below the normal range may be flushed)
      bar  = e_Ga + p e_sumGa + |sumGa| e_p + U |p sumGa| + U |dx| + 2^-149.
    The bar is relative class by class: a class clamped by the log-softmax gate has Ga = 0 and dx = -p sumGa, of the order 1e-31 and
    below, and is held to that size, which is what makes a dropped gate visible (below).
  * arg-max maps (x0_recon over clamp(a) with the -70 of [MASK]; xt1_recon over lm): compared where the reference's top-two gap exceeds
    the sum of the two values' bars; the positions left out are counted and recorded, at most 2 % of a case (CPU test).

CLAMP EDGES.  A class whose fp64 pre-clamp value lies within its own bar of -70 or 0 has an undecidable gate, and a flipped gate
changes the whole row through GS and sumGa: the dlogits rows that hold such a class are left out (at most 2 % of the rows of a case, never
all rows of a sample: CPU test on the reference alone).  One edge is decidable and not counted: a <= 0 holds exactly in the reference
and in the kernel (the row sum holds the term exp(0) = 1 exactly, so lse >= max and x - lse <= 0 after rounding too): the upper
log-softmax gate is open in both.
Measured on the CPU in fp64 (T = 100, K in {32, 260, 4096}, t in {0, 1, 37, 99}, 64 positions each, half of them masked, a few with
x_t != x_0): with 3 randn logits no row comes within 1e-4 of either edge; the lower clamp of the posterior is active on about half the
rows of the t = 0 sample (class [MASK] of the unmasked positions: LOG_ZERO twice) and on none at t >= 1; a row with one logit raised to
120 clamps every other class's log-softmax well below -70 at t >= 1 without an edge row, while at t = 0, and at t >= 1 where the raised
class is an unmasked x_t, the row sits exactly on pre = 0.  So every case has spread rows in its t = 0 sample and peaked rows (never
at an unmasked x_t) in the others: both gates are evaluated on both sides.  The upper clamp of the posterior never activated in these
measurements, and no input is invented for it.
The committed inputs themselves (asserted by the CPU tests below): no edge row and no undecided arg-max position in any of the 18 cases;
the log-softmax clamp is active on 14 of the 111 rows of a class-width case (300 of 1616 in the main case), the posterior's lower clamp
on 19 to 28 of them (50 of 1616).
What the posterior gate can change: with the product's schedule a model value pre_k < -70 arises only from LOG_ZERO twice -- class [MASK]
at an unmasked position -- where the true posterior carries the same factor, so |G_K| <= g e^-54; and at t = 0 (rho = 1 exactly: the
t - 1 wrap reads log 0) GS = 0 whatever the gate says.  There the gate is evaluated but inert: no f32 output can show a gate that is
ignored.  The kernels take the eight schedule buffers as plain arrays, so the case `gate` (K = 4, t = 0, 10, 5) feeds them a synthetic
set -- log_cumprod_bt = -66 at every t, log_bt lowered by 50, log_at lowered by 1 -- and raises the logit of an unmasked x_t to 120:
S_m stays near -log_cumprod_at, class [MASK] of those rows has pre = LOG_ZERO + log_cumprod_ct[t - 1] + S_m < -71 while the truth's
S_t = 66 keeps e^ltr_K near 4e-3, and the row's own pre at x_t is -1, not 0.  Its gradient then depends on the gate by 1e-2 of its size,
with no edge row; the same buffers push pre decidedly above 0 on 15 spread rows (gate_counts in the parity report), so the upper side
of the gate is evaluated as well.  This is the posterior gate with consequences, on the GPU and in the injected-fault test.

THE STEP AND q_sample (section "step" below) keep the references the suite already trusts: posterior and x0 hooks against oracle.d3pm
(predict_start_from_logits, cf_mix, q_posterior; atol 2e-5 as test_step_kernel_full_width_matches_oracle, 2e-4 for the x0 hook as
test_reverse_step_matches_reference), tokens against gumbel_argmax wherever the oracle's top-two margin of gumbel + posterior exceeds
1e-3 (test_reverse_step_matches_reference's margin); the fp32 restatement is the reference by design: the step's contract is bit-equal
tokens.  Low-margin positions are at most 1 % of a case (CPU test on the oracle alone, for the committed seeds).

The main case is the issue's B = 16, L = 101: 1616 positions, which IS a multiple of 4; the wave-level `pos >= B L` exit is taken in
every case of the class-width family (3 x 37 = 111 positions), to which K = 4096 is added so that the FULL instantiations take it too.

Every case records the worst error / bar ratio of every output with tests.conftest.parity_report (objective_kernels::*).  Outputs are
views into sentinel-filled buffers (a stray wave writes K floats past dlogits, a row of probs past its end): all stay intact bit for bit.

The CPU part (not marked gpu) tests this file's own machinery: the explicit gradient chain the bars are computed from equals autograd;
an f32 emulation of the arithmetic (plain exp / log in f32, fp64 row sum) meets every bar on the committed inputs, so the bars are not
below fp32's own noise; each of nine injected faults lands above a bar; the leave-out shares hold."""
import functools
import math

import numpy as np
import pytest
import torch

from tests.conftest import parity_report

gpu = pytest.mark.gpu

U = 2.0 ** -24
CE = 1.7e-7 + U
EG = 8 * U
FLUSH = 2.0 ** -126
LZ32 = float(np.float32(math.log(1e-30)))
C01, C09 = float(np.float32(0.1)), float(np.float32(0.9))
SENT = -7777
T = 100
SCHED_ORDER = ("log_at", "log_bt", "log_ct", "log_1_min_ct", "log_cumprod_at", "log_cumprod_bt", "log_cumprod_ct", "log_1_min_cumprod_ct")
FAMILY_K = [4, 252, 256, 260, 1024, 4092, 4096, 4100, 8192]
STEP_K = [4, 252, 256, 260, 512, 1024, 2048, 4092, 4100, 8192]
FAULTS = ["no_aux_grad", "no_adaptive", "mw1_is_1", "no_post_gate", "no_lsm_gate", "miss_at_xt", "no_mask_in_S", "t0_row0", "lt_prebatch"]


def gam(k):
    return U * (8 + 2 * math.sqrt(k))


def f32(v):
    return float(np.float32(v))


# ----------------------------------------------------------------------------- inputs
def schedule(K, synthetic=False):
    from oracle import d3pm as od
    sd = od.schedule_buffers(T, K)
    s = [sd[n].clone() for n in SCHED_ORDER]
    if synthetic:                                   # see "What the posterior gate can change" above
        s[5] = torch.full_like(s[5], -66.0)
        s[5][T] = -math.inf                         # (the t - 1 wrap row stays log 0)
        s[1] = s[1] - 50.0
        s[0] = s[0] - 1.0
    return s


def tokens(K, B, L, t, g):
    """x0, xt (B, L): half the positions [MASK]; unmasked ones equal to x0 except: x_t != x_0 in the same register quad (j = k >> 8) and
    lane, in the same quad and another lane, in another quad; tokens 0 and K - 1 (first and last quad) and x0 = K, masked and not."""
    x0 = torch.randint(0, K, (B, L), generator=g)
    xt = x0.clone()
    xt[torch.rand(B, L, generator=g) < 0.5] = K
    for b in range(B if L > 10 else 0):
        def put(l, v0, vt):
            x0[b, l], xt[b, l] = v0, vt
        base = int(x0[b, 0])
        other_lane = (base & ~255) | ((base + 8) & 255)
        put(0, base, base ^ 1)                                              # same quad, same lane
        put(1, base, other_lane if other_lane < K else (base + 2) % K)      # same quad, another lane
        put(2, base, (base + 256 + 5) % K)                                  # another quad (K > 256)
        put(3, 0, K - 1)
        put(4, K - 1, 0)
        put(5, K - 1, K - 1)
        put(6, 0, K)
        put(7, K, K)
        put(8, K, (base + 1) % K)
        put(9, K - 1, K)
        put(10, 0, 0)
    xt.clamp_(max=K)
    return x0, xt


def peaked_logits(K, B, L, t, x0, xt, g, semi=False):
    """3 randn logits; in the samples with t >= 1 every fifth position has one logit raised to 120 (class x_0, or another one where x_0
    is an unmasked x_t or [MASK]).  semi (case `gate`): unmasked positions raise class x_t by 14 instead."""
    x = 3.0 * torch.randn(B, L, K, generator=g)
    for b in range(B):
        if int(t[b]) == 0:
            continue
        for l in range(2, L, 5):
            c, ct = int(x0[b, l]), int(xt[b, l])
            if semi and ct != K:
                x[b, l, ct] = 120.0
                continue
            if c == K:
                c = l % K
            if c == ct:
                c = (c + 1) % K
            x[b, l, c] = 120.0
    return x


def make_case(name):
    """name -> dict of CPU tensors and settings (committed inputs: everything comes from the seed below)"""
    kind, _, arg = name.partition(":")
    mw, auxw, adaptive, synthetic = (1.0, 0.7), 5e-4, True, False
    if kind == "main":                               # arg: adaptive | plain | noaux
        K, B, L = 4096, 16, 101
        t = [0, 1, T - 1, 37, 37, 2, 5, 11, 23, 42, 58, 64, 71, 80, 93, 98]
        adaptive = arg != "plain"
        auxw = 0.0 if arg == "noaux" else 5e-4
        seed = 1
    elif kind == "family":
        K, B, L = int(arg), 3, 37
        t = [0, 1, T - 1]
        seed = 100 + K
    elif kind == "gate":
        K, B, L = 4, 3, 37
        t = [0, 10, 5]
        synthetic = True
        seed = 50
    elif kind == "fin":                              # arg: B x L
        B, L = (int(v) for v in arg.split("x"))
        K = 8
        if B == 1024:
            t = [(7 * b * b + 3 * b) % T for b in range(B)]
        else:
            t = ([7, 7, 0, 7, 93, 93, 1, T - 1] * B)[:B]    # three clips share t = 7, two share t = 93
        seed = 1000 + B + L
    else:
        raise KeyError(name)
    g = torch.Generator().manual_seed(seed)
    t = torch.tensor(t, dtype=torch.int64)
    x0, xt = tokens(K, B, L, t, g)
    logits = peaked_logits(K, B, L, t, x0, xt, g, semi=synthetic)
    pt = (0.004 + 0.012 * torch.rand(B, generator=g)).float()          # distinct per clip
    h0 = torch.rand(T, generator=g).float() * 50 + 0.5
    c0 = torch.randint(0, 20, (T,), generator=g).float()
    return dict(name=name, K=K, B=B, L=L, t=t, x0=x0, xt=xt, logits=logits.float().contiguous(), pt=pt, h0=h0, c0=c0,
                sched=schedule(K, synthetic), mw=(f32(mw[0]), f32(mw[1])), auxw=f32(auxw), adaptive=adaptive)


MAIN_CASES = ["main:adaptive", "main:plain", "main:noaux"]
FAMILY_CASES = [f"family:{K}" for K in FAMILY_K] + ["gate"]
FIN_CASES = ["fin:5x1", "fin:8x37", "fin:6x256", "fin:5x300", "fin:1024x1"]
ALL_CASES = MAIN_CASES + FAMILY_CASES + FIN_CASES
FAULT_CASES = ["family:4", "family:260", "gate", "fin:8x37"]


# ----------------------------------------------------------------------------- the objective: one statement, two precisions
def lae(a, b):
    return torch.maximum(a, b) + torch.log1p(torch.exp(-(a - b).abs()))


def forward(c, x, dt, fault=None):
    """The objective per position from logits x (B, L, K) of dtype dt (fp64: the reference, differentiable; f32: the emulation, whose
    log-softmax row sum is fp64 as the kernel's).  -> dict of everything the tail, the gradient chain and the bars need."""
    K, B, L = c["K"], c["B"], c["L"]
    dev = x.device
    sc = [s.to(dev).to(dt) for s in c["sched"]]
    t, x0, xt = c["t"].to(dev), c["x0"].to(dev), c["xt"].to(dev)
    tp = (t - 1 + (T + 1)) % (T + 1)
    if fault == "t0_row0":
        tp = torch.where(t == 0, torch.zeros_like(t), tp)
    s_ = lambda i, idx: sc[i][idx].view(B, 1, 1)
    la, lb, lc, lca, lcb, lcc = s_(0, t), s_(1, t), s_(2, t), s_(4, t), s_(5, t), s_(6, t)
    pca, pcb, pcc, p1mcc = s_(4, tp), s_(5, tp), s_(6, tp), s_(7, tp)
    LZ = torch.tensor(LZ32, dtype=dt, device=dev)
    zero, one = torch.zeros((), dtype=dt, device=dev), torch.ones((), dtype=dt, device=dev)
    qt_hit, qt_miss = lae(lca, lcb), lae(LZ + lca, lcb)
    q1_hit, q1_miss = lae(la, lb), lae(LZ + la, lb)
    xd = x.double()
    a = (xd - torch.logsumexp(xd, -1, keepdim=True)).to(dt)
    r = a.clamp(-70, 0)
    kk = torch.arange(K, device=dev)
    masked = (xt == K).unsqueeze(-1)
    is_xt, is_x0 = kk == xt.unsqueeze(-1), kk == x0.unsqueeze(-1)
    hit = torch.zeros_like(is_xt) if fault == "miss_at_xt" else is_xt
    lqt = torch.where(masked, lcc, torch.where(hit, qt_hit, qt_miss))
    lq1 = torch.where(masked, lc, torch.where(hit, q1_hit, q1_miss))
    lq1f = torch.cat([lq1, torch.where(masked, zero, LZ)], -1)
    lx0 = torch.where(is_x0, zero, LZ)
    E30 = torch.exp(LZ)
    w0 = torch.where(is_x0, one, E30)
    w0f = torch.cat([w0, torch.where((x0 == K).unsqueeze(-1), one, E30)], -1)
    alpha = torch.cat([pca.expand(B, L, K), p1mcc.expand(B, L, 1)], -1)
    beta = torch.cat([pcb.expand(B, L, K), pcc.expand(B, L, 1)], -1)

    def post(qk):
        q = torch.cat([qk, LZ.expand(B, L, 1)], -1)
        S = torch.logsumexp(q[..., :K] if fault == "no_mask_in_S" else q, -1, keepdim=True)
        qn = q - S
        e = lae(qn + alpha, beta)
        return dict(q=q, S=S, qn=qn, e=e, pre=(e + lq1f) + S)

    M, R = post(r - lqt), post(lx0 - lqt)
    lm, ltr = M["pre"].clamp(-70, 0), R["pre"].clamp(-70, 0)
    eltr = ltr.exp()
    mw1 = 1.0 if fault == "mw1_is_1" else c["mw"][1]
    mw = torch.where(masked, c["mw"][0] * one, mw1 * one)                # (B, L, 1)
    klt, nllt, auxt = eltr * (ltr - lm), w0f * lm, w0 * (lx0 - r)
    rc = torch.cat([r, torch.full_like(r[..., :1], -70.0)], -1)
    return dict(a=a, r=r, rc=rc, lqt=lqt, lq1f=lq1f, lx0=lx0, w0=w0, w0f=w0f, alpha=alpha, masked=masked, M=M, R=R, lm=lm, ltr=ltr,
                eltr=eltr, mw=mw, klt=klt, nllt=nllt, auxt=auxt,
                kl=klt.sum(-1) * mw[..., 0], nll=-nllt.sum(-1), aux=auxt.sum(-1) * mw[..., 0],
                probs=lm.exp().permute(0, 2, 1), x0_recon=rc.argmax(-1), xt1_recon=lm.argmax(-1),
                consts=(qt_hit, qt_miss, q1_hit, q1_miss))


def weights(c, dt, dev, fault=None):
    """per-sample scalars (B,): m0, w (adaptive weight), aux_weight, pt"""
    t = c["t"].to(dev)
    m0 = (t == 0).to(dt)
    if c["adaptive"] and fault != "no_adaptive":
        w = (1 - t.to(dt) / T) + 1.0
    else:
        w = torch.ones_like(m0)
    return m0, w, torch.tensor(c["auxw"], dtype=dt, device=dev), c["pt"].to(dev).to(dt)


def tail(c, F, dt, fault=None):
    """The finalize kernel: per-sample reductions, loss, Lt_history / Lt_count in sample order."""
    B, L = c["B"], c["L"]
    dev = F["kl"].device
    m0, w, auxw, pt = weights(c, dt, dev, fault)
    kls, nlls, auxs = F["kl"].sum(-1), F["nll"].sum(-1), F["aux"].sum(-1)
    kl_loss = m0 * nlls + (1 - m0) * kls
    vb = kl_loss / pt
    aux_part = torch.zeros_like(vb)
    if c["auxw"] != 0:
        aux_part = w * auxw * (m0 * nlls + (1 - m0) * auxs) / pt
        vb = vb + aux_part
    loss = vb.sum() / (float(B) * float(L))
    acc = (F["x0_recon"] == c["x0"].to(dev)).to(dt).sum(-1) / L
    keep = (F["xt1_recon"] == c["xt"].to(dev)).to(dt).sum(-1) / L
    nd = np.float32 if dt == torch.float32 else np.float64
    h, cnt = c["h0"].numpy().astype(nd), c["c0"].numpy().astype(nd)
    h_pre = h.copy()
    kln = kl_loss.detach().cpu().numpy().astype(nd)
    for b, tb in enumerate(c["t"].tolist()):
        base = h_pre[tb] if fault == "lt_prebatch" else h[tb]
        h[tb] = nd(C01) * (kln[b] * kln[b]) + nd(C09) * base
        cnt[tb] += nd(1)
    return dict(loss=loss.reshape(1), per_sample=torch.stack([kl_loss, vb, acc, keep], 1), Lt_history=torch.from_numpy(h),
                Lt_count=torch.from_numpy(cnt), kl_loss=kl_loss, vb=vb, aux_part=aux_part, sums=(kls, nlls, auxs))


def chain(c, F, dt, fault=None):
    """d loss / d logits by the kernel's hand-derived chain (header comment of d3pm_train_bwd_kernel), from forward()'s values."""
    K, B, L = c["K"], c["B"], c["L"]
    dev = F["a"].device
    m0, w, auxw, pt = (v.view(-1, 1, 1) if v.ndim else v for v in weights(c, dt, dev, fault))
    inv = 1.0 / (pt * float(B) * float(L))
    mw = F["mw"]
    g_kl, g_nll, g_aux = (1 - m0) * mw * inv, m0 * (1 + w * auxw) * inv * torch.ones_like(mw), (1 - m0) * w * auxw * mw * inv
    if fault == "no_aux_grad":
        g_aux = torch.zeros_like(g_aux)
    M, a = F["M"], F["a"]
    G = -(g_kl * F["eltr"] + g_nll * F["w0f"])
    gate_p = (M["pre"] >= -70) & (M["pre"] <= 0)
    if fault == "no_post_gate":
        gate_p = torch.ones_like(gate_p)
    Ge = torch.where(gate_p, G, torch.zeros_like(G))
    rho = torch.exp((M["qn"] + F["alpha"]) - M["e"])
    Gqn = Ge * rho
    GS = Ge.sum(-1, keepdim=True) - Gqn.sum(-1, keepdim=True)
    pi = torch.exp(M["qn"][..., :K])
    Gr = (Gqn[..., :K] + GS * pi) - g_aux * F["w0"]
    gate_a = (a >= -70) & (a <= 0)
    if fault == "no_lsm_gate":
        gate_a = torch.ones_like(gate_a)
    Ga = torch.where(gate_a, Gr, torch.zeros_like(Gr))
    sGa = Ga.sum(-1, keepdim=True)
    p = torch.exp(a)
    return dict(dx=Ga - p * sGa, G=G, Ge=Ge, gate_p=gate_p, rho=rho, Gqn=Gqn, GS=GS, pi=pi, Gr=Gr, gate_a=gate_a, Ga=Ga, sGa=sGa, p=p,
                g=(g_kl, g_nll, g_aux))


def emulate(c, fault=None, dev="cpu"):
    """f32 emulation of the three kernels (optionally with an injected fault) -> the kernels' outputs"""
    with torch.no_grad():
        F = forward(c, c["logits"].to(dev), torch.float32, fault)
        Tl = tail(c, F, torch.float32, fault)
        Ch = chain(c, F, torch.float32, fault)
    return dict(kl=F["kl"], nll=F["nll"], aux=F["aux"], probs=F["probs"], x0_recon=F["x0_recon"], xt1_recon=F["xt1_recon"],
                loss=Tl["loss"], per_sample=Tl["per_sample"], Lt_history=Tl["Lt_history"], Lt_count=Tl["Lt_count"], dlogits=Ch["dx"])


# ----------------------------------------------------------------------------- reference values and bars
def post_bars(P, e_qk, alpha, lq1f, e_lq1f, K):
    """bars of one posterior evaluation (dict of post()): e_pre, e_S, e_qn, rho"""
    q, S, qn, e, pre = P["q"], P["S"], P["qn"], P["e"], P["pre"]
    e_q = torch.cat([e_qk, torch.zeros_like(e_qk[..., :1])], -1)
    pi = qn.exp()
    dd = (q - q.max(-1, keepdim=True).values).abs()
    e_S = (pi * (e_q + CE * dd + 2 * U)).sum(-1, keepdim=True) + gam(K + 1) + 4 * U + U * S.abs()
    rho = torch.exp((qn + alpha) - e)
    e_pre = rho * (e_q + U * qn.abs() + U * (qn + alpha).abs()) + e_S + U * e.abs() + 8 * U + e_lq1f + U * (e + lq1f).abs() + U * pre.abs()
    return dict(e_pre=e_pre, e_S=e_S, e_qn=e_q + e_S + U * qn.abs(), rho=rho, e_q=e_q)


def top2_decided(v, e_v):
    """positions (...,) whose arg-max over the last axis is decided: top-two gap above the two values' bars"""
    top, idx = v.topk(2, -1)
    return (top[..., 0] - top[..., 1]) > e_v.gather(-1, idx).sum(-1)


def reference(c, dev="cpu", grad=True):
    """fp64 values of every output of the three kernels, their bars, the decided arg-max positions and the dlogits rows kept."""
    K, B, L = c["K"], c["B"], c["L"]
    dt = torch.float64
    x = c["logits"].to(dev).double().requires_grad_(grad)
    F = forward(c, x, dt)
    Tl = tail(c, F, dt)
    R = {}
    if grad:
        R["dlogits"] = torch.autograd.grad(Tl["loss"].sum(), x)[0]
    with torch.no_grad():
        F = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in F.items()}
        F["M"] = {k: v.detach() for k, v in F["M"].items()}
        Ch = chain(c, F, dt)
        a, M, Rt, masked = F["a"], F["M"], F["R"], F["masked"]
        xd = x.detach()
        p = Ch["p"]
        e_lse = (p * (CE * (xd - xd.max(-1, keepdim=True).values).abs() + 2 * U)).sum(-1, keepdim=True) + 2 * U
        e_a = e_lse + U * a.abs()
        e_c = lambda v: torch.where(masked, torch.zeros_like(v), 2 * U * v.abs() + 8 * U)
        e_lqt = e_c(F["lqt"])
        e_lq1f = torch.cat([e_c(F["lq1f"][..., :K]), torch.zeros_like(e_lse)], -1)
        bm = post_bars(M, e_a + e_lqt + U * M["q"][..., :K].abs(), F["alpha"], F["lq1f"], e_lq1f, K)
        bt = post_bars(Rt, e_lqt + U * Rt["q"][..., :K].abs(), F["alpha"], F["lq1f"], e_lq1f, K)
        e_lm, e_ltr = bm["e_pre"], bt["e_pre"]
        lm, ltr, eltr, mw = F["lm"], F["ltr"], F["eltr"], F["mw"][..., 0]
        # ---- forward, per position
        dl = (ltr - lm).abs()
        e_klt = eltr * ((e_ltr + 2 * U) * dl + e_ltr + e_lm + U * dl) + U * F["klt"].abs()
        R["kl"], R["nll"], R["aux"] = F["kl"], F["nll"], F["aux"]
        R["bar_kl"] = (e_klt.sum(-1) + gam(K + 1) * F["klt"].abs().sum(-1)) * mw + U * F["kl"].abs()
        R["bar_nll"] = (F["w0f"] * (e_lm + 6 * U * lm.abs())).sum(-1) + gam(K + 1) * F["nllt"].abs().sum(-1) + U * F["nll"].abs()
        R["bar_aux"] = ((F["w0"] * (e_a + U * (F["lx0"] - F["r"]).abs()) + 5 * U * F["auxt"].abs()).sum(-1)
                        + gam(K) * F["auxt"].abs().sum(-1)) * mw + U * F["aux"].abs()
        R["probs"] = F["probs"]
        R["bar_probs"] = (lm.exp() * (e_lm + 2 * U)).permute(0, 2, 1) + 2.0 ** -149
        R["x0_recon"], R["xt1_recon"] = F["x0_recon"], F["xt1_recon"]
        R["dec0"] = top2_decided(F["rc"], torch.cat([e_a, torch.zeros_like(e_lse)], -1))
        R["dec1"] = top2_decided(lm, e_lm)
        # ---- finalize
        m0, w, auxw, pt = weights(c, dt, dev)
        sums_bar = []
        for v, bar in ((F["kl"], R["bar_kl"]), (F["nll"], R["bar_nll"]), (F["aux"], R["bar_aux"])):
            sums_bar.append(bar.sum(-1) + gam(L) * v.abs().sum(-1))
        e_kls, e_nlls, e_auxs = sums_bar
        e_kll = m0 * e_nlls + (1 - m0) * e_kls
        kl_loss, vb = Tl["kl_loss"].detach(), Tl["vb"].detach()
        e_vb = e_kll / pt + 2 * U * (kl_loss / pt).abs() + U * vb.abs()
        if c["auxw"] != 0:
            e_vb = e_vb + w * auxw * (m0 * e_nlls + (1 - m0) * e_auxs) / pt + 6 * U * Tl["aux_part"].detach().abs()
        und0, und1 = (~R["dec0"]).sum(-1).double(), (~R["dec1"]).sum(-1).double()
        R["per_sample"] = Tl["per_sample"].detach()
        R["bar_per_sample"] = torch.stack([e_kll + 2.0 ** -149, e_vb + 2.0 ** -149, und0 / L + 2 * U, und1 / L + 2 * U], 1)
        R["loss"] = Tl["loss"].detach()
        R["bar_loss"] = (e_vb.sum() + gam(B) * vb.abs().sum()) / (B * L) + 3 * U * R["loss"].abs()
        kln, ekn = kl_loss.cpu().numpy(), e_kll.cpu().numpy()
        h = c["h0"].numpy().astype(np.float64)
        e_h = np.zeros(T)
        for b, tb in enumerate(c["t"].tolist()):
            h[tb] = C01 * kln[b] ** 2 + C09 * h[tb]
            e_h[tb] = C01 * (2 * abs(kln[b]) * ekn[b] + ekn[b] ** 2 + U * kln[b] ** 2) + C09 * e_h[tb] + 3 * U * abs(h[tb])
        assert np.array_equal(h, Tl["Lt_history"].numpy())
        R["Lt_history"], R["bar_Lt_history"] = torch.from_numpy(h).to(dev), torch.from_numpy(e_h).to(dev)
        R["Lt_count"] = Tl["Lt_count"].to(dev)
        # ---- clamp edges
        pre = M["pre"]
        edge = ((a + 70).abs() <= e_a).any(-1) | ((pre + 70).abs() <= e_lm).any(-1) | (pre.abs() <= e_lm).any(-1)
        R["keep_rows"] = ~edge
        R["gate_counts"] = dict(lsm_low=int((a < -70).any(-1).sum()), post_low=int((pre < -70).any(-1).sum()),
                                post_high=int((pre > 0).any(-1).sum()), edge_rows=int(edge.sum()))
        # ---- dlogits
        if grad:
            G, Ge, rho, Gqn, GS, pi, Gr, Ga, sGa = (Ch[k] for k in ("G", "Ge", "rho", "Gqn", "GS", "pi", "Gr", "Ga", "sGa"))
            g_kl, g_nll, g_aux = Ch["g"]
            zp, za = torch.zeros_like(G), torch.zeros_like(Gr)
            e_G = torch.where(Ch["gate_p"], G.abs() * (EG + 5 * U) + g_kl * eltr * e_ltr, zp)
            qa = M["qn"] + F["alpha"]
            e_lrho = (1 - rho) * (bm["e_qn"] + U * qa.abs()) + U * M["e"].abs() + 8 * U + U * (qa - M["e"]).abs() + 2 * U
            e_Gqn = Ge.abs() * rho * e_lrho + rho * e_G + U * Gqn.abs()
            e_GS = (e_G.sum(-1, keepdim=True) + e_Gqn.sum(-1, keepdim=True)
                    + gam(K + 1) * (Ge.abs().sum(-1, keepdim=True) + Gqn.abs().sum(-1, keepdim=True)) + U * GS.abs())
            e_pi = pi * (bm["e_qn"][..., :K] + 2 * U)
            e_Gr = (e_Gqn[..., :K] + GS.abs() * e_pi + pi * e_GS + U * (GS * pi).abs() + U * (Gqn[..., :K] + GS * pi).abs()
                    + g_aux * F["w0"] * (EG + 4 * U) + U * Gr.abs())
            e_Ga = torch.where(Ch["gate_a"], e_Gr, za)
            e_sGa = e_Ga.sum(-1, keepdim=True) + gam(K) * Ga.abs().sum(-1, keepdim=True)
            e_p = p * (CE * a.abs() + e_a + 2 * U) + FLUSH
            R["bar_dlogits"] = e_Ga + p * e_sGa + sGa.abs() * e_p + U * (p * sGa).abs() + U * Ch["dx"].abs() + 2.0 ** -149
            R["chain_dx"] = Ch["dx"]
    return R


def ratio(got, want, bar):
    """worst |got - want| / bar (a non-finite result counts as infinitely wrong)"""
    got = got.double().to(want.device)
    if got.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(got).all()):
        return math.inf
    err = (got - want).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / bar).max())


def compare(got, R):
    """worst error / bar ratio of every output in `got` (a dict with the kernels' output names) -> dict"""
    res = {}
    for k in ("kl", "nll", "aux", "probs", "loss", "Lt_history"):
        if got.get(k) is not None:
            res[k] = ratio(got[k], R[k], R["bar_" + k])
    if got.get("per_sample") is not None:
        for i, n in enumerate(("kl_loss", "vb", "acc_rate", "keep_rate")):
            res[n] = ratio(got["per_sample"][:, i], R["per_sample"][:, i], R["bar_per_sample"][:, i])
    if got.get("Lt_count") is not None:
        res["Lt_count"] = 0.0 if torch.equal(got["Lt_count"].double().cpu(), R["Lt_count"].double().cpu()) else math.inf
    for k, dec in (("x0_recon", "dec0"), ("xt1_recon", "dec1")):
        if got.get(k) is not None:
            bad = (got[k].to(R[k].device) != R[k]) & R[dec]
            res[k] = math.inf if bool(bad.any()) else 0.0
    if got.get("dlogits") is not None:
        keep = R["keep_rows"]
        res["dlogits"] = ratio(got["dlogits"].view(R["dlogits"].shape)[keep], R["dlogits"][keep], R["bar_dlogits"][keep])
    return res


@functools.lru_cache(maxsize=None)
def cpu_case(name):
    c = make_case(name)
    return c, reference(c, "cpu")


# ----------------------------------------------------------------------------- CPU: the test's own machinery
@pytest.mark.parametrize("name", ALL_CASES)
def test_reference_leave_out_shares_and_gate_coverage(name):
    """On the reference alone: at most 2 % of the dlogits rows of a case hold a clamp-edge class, no sample loses all its rows, at most
    2 % of the positions have an undecided arg-max; the explicit chain the bars are built on equals autograd on the rows kept; and the
    class-width cases evaluate both gates on both sides (log-softmax clamp active on peaked rows, posterior clamp on the t = 0 rows)."""
    c, R = cpu_case(name)
    n = c["B"] * c["L"]
    keep = R["keep_rows"]
    cap = max(int(0.02 * n), 0)
    assert int((~keep).sum()) <= cap, R["gate_counts"]
    assert bool(keep.any(-1).all()), "a sample lost all its rows"
    assert int((~R["dec0"]).sum()) <= cap and int((~R["dec1"]).sum()) <= cap
    scale = R["dlogits"].abs().amax(-1, keepdim=True)
    assert float(((R["chain_dx"] - R["dlogits"]).abs() / scale)[keep].max()) < 1e-9
    if not name.startswith("fin"):
        gc = R["gate_counts"]
        assert gc["lsm_low"] > 0 and gc["post_low"] > 0, gc
        assert int((c["x0"] == c["K"]).sum()) > 0 and int((c["xt"] == c["K"] - 1).sum()) > 0 and int((c["x0"] == 0).sum()) > 0


@pytest.mark.parametrize("name", ALL_CASES)
def test_f32_emulation_meets_every_bar(name):
    """The bars are not below fp32's own noise: plain f32 arithmetic (fp64 row sum) passes them all on the committed inputs."""
    c, R = cpu_case(name)
    res = compare(emulate(c), R)
    assert max(res.values()) <= 1, res


@pytest.mark.parametrize("fault", FAULTS)
def test_injected_fault_lands_above_a_bar(fault):
    caught = {}
    for name in FAULT_CASES:
        c, R = cpu_case(name)
        res = compare(emulate(c, fault), R)
        caught[name] = {k: v for k, v in res.items() if v > 1}
    assert any(caught.values()), f"{fault}: no output of any case above its bar"
    print(fault, {n: sorted(v) for n, v in caught.items()})


# ----------------------------------------------------------------------------- the step and q_sample: inputs and oracle results
STEP_B, STEP_L, STEP_ROW0 = 3, 37, 1000


def gumbel_margin(logp, seed, stream):
    """oracle tokens of gumbel + logp (B, K+1, L) and the top-two margin of that sum per position"""
    from oracle import d3pm as od, philox
    B, K1, L = logp.shape
    u = torch.from_numpy(philox.uniform_bkl(seed, stream, B, K1, L, row0=STEP_ROW0))
    top = (-torch.log(-torch.log(u + 1e-30) + 1e-30) + logp).topk(2, 1).values
    return od.gumbel_argmax(logp, seed, stream, row0=STEP_ROW0), top[:, 0] - top[:, 1]


@functools.lru_cache(maxsize=None)
def step_case(K, guided):
    """masked and unmasked x_t, x_t in the last quad, t in {0, 1, T - 1}, 111 positions, row0 = 1000 (committed seeds: 4321 + K)"""
    from oracle import d3pm as od
    B, L = STEP_B, STEP_L
    g = torch.Generator().manual_seed(7000 + K)
    lc = torch.randn(B, K, L, generator=g) * 3.0
    lu = lc + torch.randn(B, K, L, generator=g)
    xt = torch.randint(0, K, (B, L), generator=g)
    xt[:, ::3] = K
    xt[:, 1], xt[:, 4], xt[0, 5] = K - 1, K - 2, 0
    t = torch.tensor([0, 1, T - 1])
    sd = od.schedule_buffers(T, K)
    rec = od.cf_mix(od.predict_start_from_logits(lc)[:, :-1], od.predict_start_from_logits(lu)[:, :-1], 2.0) if guided \
        else od.predict_start_from_logits(lc)
    post = od.q_posterior(rec, od.index_to_log_onehot(xt, K + 1), t, sd)
    tok, margin = gumbel_margin(post, 4321 + K, 7)
    return dict(K=K, lc=lc, lu=lu if guided else None, xt=xt, t=t, sd=sd, rec=rec, post=post, tok=tok, margin=margin, seed=4321 + K, stream=7)


@functools.lru_cache(maxsize=None)
def q_sample_case(K):
    from oracle import d3pm as od
    B, L = STEP_B, STEP_L
    g = torch.Generator().manual_seed(9000 + K)
    x0 = torch.randint(0, K, (B, L), generator=g)
    x0[:, ::7] = K
    x0[:, 1], x0[:, 2] = K - 1, 0
    t = torch.tensor([5, 1, T - 1])
    sd = od.schedule_buffers(T, K)
    tok, margin = gumbel_margin(od.q_pred(od.index_to_log_onehot(x0, K + 1), t, sd), 4321 + K, 9)
    return dict(K=K, x0=x0, t=t, sd=sd, tok=tok, margin=margin, seed=4321 + K, stream=9)


LOW_MARGIN_CAP = int(0.01 * STEP_B * STEP_L)


@pytest.mark.parametrize("K", STEP_K + [4096])
def test_low_margin_positions_of_the_committed_seeds(K):
    """On the oracle alone: at most 1 % of the positions of a step / q_sample case have a top-two margin of gumbel + log-probability
    within 1e-3 (where a token may legitimately differ)."""
    for case in (step_case(K, True), step_case(K, False), q_sample_case(K)):
        assert int((case["margin"] <= 1e-3).sum()) <= LOW_MARGIN_CAP
        assert case["tok"].shape == (STEP_B, STEP_L) and (STEP_B * STEP_L) % 4 != 0


# ----------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    gsdd_amd.lib()
    assert tuple(gsdd_amd.d3pm.SCHED_ORDER) == SCHED_ORDER
    return gsdd_amd


def guarded(shape, dtype, before, after, fill=None):
    """-> (buffer, view): a contiguous view of `shape` with `before` / `after` sentinel elements around it (the view holds the sentinel
    too unless `fill` is given)"""
    n = int(np.prod(shape))
    buf = torch.full((before + n + after,), SENT, dtype=dtype, device="cuda")
    v = buf[before:before + n].view(shape)
    if fill is not None:
        v.copy_(fill)
    return buf, v, before, n


def intact(entry):
    buf, _, before, n = entry
    return bool((buf[:before] == SENT).all()) and bool((buf[before + n:] == SENT).all())


def dev_inputs(c):
    cu = lambda v: v.cuda().contiguous()
    return dict(logits=cu(c["logits"].view(c["B"] * c["L"], c["K"])), x0=cu(c["x0"]), xt=cu(c["xt"]), t=cu(c["t"]), pt=cu(c["pt"]),
                sched=[cu(s) for s in c["sched"]])


def run_objective(G, c, D, which, probs=False):
    """One call of gsdd_d3pm_train_loss ("loss"), gsdd_d3pm_train_loss_bwd ("bwd") or gsdd_d3pm_train_loss_grad ("grad") through
    ops.lib() with a TrainDesc whose every output is a view into a sentinel-filled buffer.
    -> (rc, outputs, all guards intact, every buffer as it was before the call)"""
    import ctypes as C
    O = G.ops
    K, B, L = c["K"], c["B"], c["L"]
    n = B * L
    f, i64 = torch.float32, torch.int64
    E = dict(kl=guarded((B, L), f, 64, 64), nll=guarded((B, L), f, 64, 64), aux=guarded((B, L), f, 64, 64),
             x0_recon=guarded((B, L), i64, 16, 16), xt1_recon=guarded((B, L), i64, 16, 16),
             per_sample=guarded((B, 4), f, 16, 16), loss=guarded((1,), f, 16, 16),
             Lt_history=guarded((T,), f, 16, 16, c["h0"]), Lt_count=guarded((T,), f, 16, 16, c["c0"]))
    if probs:
        E["probs"] = guarded((B, K + 1, L), f, 64, (K + 1) * L + 64)           # a position past B L lands in "sample B"
    if which != "loss":
        E["dlogits"] = guarded((n, K), f, 64, 4 * K + 64)                      # four stray waves: four rows
    before = {k: e[0].clone() for k, e in E.items()}
    d = O.TrainDesc()
    d.logits, d.x0, d.xt, d.t_dev, d.pt = O.ptr(D["logits"]), O.ptr(D["x0"]), O.ptr(D["xt"]), O.ptr(D["t"]), O.ptr(D["pt"])
    d.B, d.L, d.K, d.T = B, L, K, T
    for i in range(8):
        d.sched[i] = O.ptr(D["sched"][i])
    d.mask_weight[0], d.mask_weight[1] = c["mw"]
    d.aux_weight, d.adaptive_aux = c["auxw"], int(c["adaptive"])
    if which != "bwd":
        for k in ("kl", "nll", "aux", "x0_recon", "xt1_recon", "Lt_history", "Lt_count", "loss", "per_sample"):
            setattr(d, k, O.ptr(E[k][1]))
    d.probs = O.ptr(E["probs"][1]) if probs else None
    if which == "loss":
        rc = O.lib().gsdd_d3pm_train_loss(C.byref(d), O.stream_ptr())
    elif which == "bwd":
        rc = O.lib().gsdd_d3pm_train_loss_bwd(C.byref(d), O.ptr(E["dlogits"][1]), O.stream_ptr())
    else:
        rc = O.lib().gsdd_d3pm_train_loss_grad(C.byref(d), O.ptr(E["dlogits"][1]), O.stream_ptr())
    torch.cuda.synchronize()
    out = {k: e[1] for k, e in E.items()}
    if which == "bwd":
        out = {"dlogits": out["dlogits"]}
    absent = torch.ones(T, dtype=torch.bool, device="cuda")
    absent[D["t"]] = False
    ok = all(intact(e) for e in E.values())
    ok = ok and bool(torch.equal(E["Lt_history"][1][absent], c["h0"].cuda()[absent])) and bool(torch.equal(E["Lt_count"][1][absent], c["c0"].cuda()[absent]))
    untouched = all(bool(torch.equal(before[k], e[0])) for k, e in E.items())
    return rc, out, ok, untouched


FWD_KEYS = ("kl", "nll", "aux", "x0_recon", "xt1_recon", "per_sample", "loss", "Lt_history", "Lt_count")


@gpu
@pytest.mark.parametrize("name", ALL_CASES)
def test_objective_kernels_match_fp64(G, name):
    """d3pm_train_loss (with and without probs), d3pm_train_loss_bwd and the fused d3pm_train_loss_grad against the fp64 reference and
    its autograd, element by element; the fused pass equal to the two kernels bit for bit; the ops wrappers equal to the raw calls;
    every sentinel intact.  main: K = 4096 (FULL), 16 clips with distinct t and pt, mask_weight (1, 0.7), adaptive / plain / aux_weight
    0.  family: J = 1 (K = 4, and 252 with an empty last lane), 256 (FULL-width J = 1, [MASK] lane wraps to lane 0), 2, 4, partial 16,
    4096, 32 partial and full (the 128 KB dynamic-LDS opt-in of the backward), 111 positions.  gate: synthetic schedule (module
    docstring).  fin: L in {1, 37, 256, 300}, B = 1024, clips sharing a t, nonzero Lt prefills."""
    c = make_case(name)
    R = reference(c, "cuda")
    D = dev_inputs(c)
    runs = {}
    for key, which, probs in (("loss_probs", "loss", True), ("loss", "loss", False), ("bwd", "bwd", False), ("grad", "grad", False)):
        rc, out, ok, _ = run_objective(G, c, D, which, probs)
        assert rc == 0, (key, G.ops.lib().gsdd_last_error().decode())
        assert ok, f"{key}: a sentinel around an output, or an Lt entry of a timestep that is not in the batch, was written"
        runs[key] = out
    rec = {"K": c["K"], "positions": c["B"] * c["L"], "edge_rows_left_out": int((~R["keep_rows"]).sum()),
           "x0_recon_left_out": int((~R["dec0"]).sum()), "xt1_recon_left_out": int((~R["dec1"]).sum()), **R["gate_counts"]}
    worst = 0.0
    for key, out in runs.items():
        for k, v in compare(out, R).items():
            rec[f"{key}.{k}"] = v
            worst = max(worst, v)
    rec["worst_ratio"] = worst
    parity_report(f"objective_kernels::{name}", rec)
    for k in FWD_KEYS:
        assert torch.equal(runs["loss"][k], runs["grad"][k]), f"fused pass differs from the loss kernel in {k}"
        assert torch.equal(runs["loss"][k], runs["loss_probs"][k]), f"the probs variant differs in {k}"
    assert torch.equal(runs["bwd"]["dlogits"], runs["grad"]["dlogits"]), "fused pass differs from the backward kernel"
    # the tensor-level wrappers
    kw = dict(K=c["K"], T=T, mask_weight=list(c["mw"]), aux_weight=c["auxw"], adaptive_aux=c["adaptive"])
    args = (D["logits"], D["x0"], D["xt"], D["t"], D["pt"], D["sched"])
    h1, c1, h2, c2 = c["h0"].cuda(), c["c0"].cuda(), c["h0"].cuda(), c["c0"].cuda()
    w_loss = G.ops.d3pm_train_loss(*args, h1, c1, want_probs=True, **kw)
    w_bwd = G.ops.d3pm_train_loss_bwd(*args, **kw)
    w_f, w_g = G.ops.d3pm_train_loss_grad(*args, h2, c2, **kw)
    for w, h, cn in ((w_loss, h1, c1), (w_f, h2, c2)):
        for k in ("loss", "per_sample", "x0_recon", "xt1_recon"):
            assert torch.equal(w[k], runs["loss"][k]), k
        assert torch.equal(h, runs["loss"]["Lt_history"]) and torch.equal(cn, runs["loss"]["Lt_count"])
    assert torch.equal(w_loss["probs"], runs["loss_probs"]["probs"])
    assert torch.equal(w_bwd.view(-1), runs["bwd"]["dlogits"].view(-1)) and torch.equal(w_g.view(-1), runs["bwd"]["dlogits"].view(-1))
    assert worst <= 1, {k: v for k, v in rec.items() if isinstance(v, float) and v > 1}


@gpu
def test_batch_above_the_finalize_limit_is_refused_with_nothing_written(G):
    """B = 1025 exceeds the finalize kernel's vb_all[1024]: gsdd_d3pm_train_loss and gsdd_d3pm_train_loss_grad return an error and
    leave every output, guard and Lt entry as it was."""
    c = make_case("fin:1025x1")
    D = dev_inputs(c)
    for which, probs in (("loss", True), ("loss", False), ("grad", False)):
        rc, _, _, untouched = run_objective(G, c, D, which, probs)
        assert rc != 0, f"{which}: B = 1025 was accepted"
        assert untouched, f"{which}: something was written before the refusal"
    parity_report("objective_kernels::refused_B1025", {"refused": True, "worst_ratio": 0.0})


def step_rows(x, K):
    return x.permute(0, 2, 1).contiguous().view(-1, K).cuda()


def run_step(G, s, hooked):
    """-> (tokens (B, L) on the CPU, guards intact, post_dbg, x0_dbg)"""
    K, B, L = s["K"], STEP_B, STEP_L
    sched = [s["sd"][n].cuda() for n in SCHED_ORDER]
    e = guarded((B, L), torch.int64, 16, 16)
    post = torch.empty((B, K + 1, L), device="cuda") if hooked else None
    x0d = torch.empty((B, K + 1, L), device="cuda") if hooked else None
    sid = torch.tensor([s["stream"]], dtype=torch.int64, device="cuda")
    G.ops.d3pm_step(step_rows(s["lc"], K), None if s["lu"] is None else step_rows(s["lu"], K), s["xt"].cuda(), e[1], sched, s["t"].cuda(),
                    sid, K=K, T=T, guidance=2.0, seed=s["seed"], row0=STEP_ROW0, post_dbg=post, x0_dbg=x0d)
    torch.cuda.synchronize()
    return e[1].cpu(), intact(e), post, x0d


@gpu
@pytest.mark.parametrize("guided", [True, False], ids=["guided", "unguided"])
@pytest.mark.parametrize("K", STEP_K)
def test_step_kernel_at_every_class_width(G, K, guided):
    """J = 1 (K = 4, 252), FULL J = 1, 2, 4, 8, 32 (K = 256, 512, 1024, 2048, 8192), partial J = 2, 16, 32 (260, 4092, 4100), hooked and
    plain instantiation of each: posterior and x0 hooks against the oracle, tokens equal to the oracle's wherever its margin exceeds
    1e-3, 111 positions (a wave of the last workgroup exits), row0 = 1000, sentinels around tok_out."""
    s = step_case(K, guided)
    hooked, ok_h, post, x0d = run_step(G, s, True)
    plain, ok_p, _, _ = run_step(G, s, False)
    assert ok_h and ok_p, "d3pm_step wrote outside tok_out"
    post_err = float((post.cpu() - s["post"]).abs().max())
    x0_err = float((x0d.cpu() - s["rec"]).abs().max())
    sure = s["margin"] > 1e-3
    mh, mp = hooked != s["tok"], plain != s["tok"]
    parity_report(f"objective_kernels::step[K{K}_{'guided' if guided else 'unguided'}]",
                  {"positions": STEP_B * STEP_L, "low_margin": int((~sure).sum()), "mismatches_hooked": int(mh.sum()),
                   "mismatches_plain": int(mp.sum()), "posterior_max_err": post_err, "x0_max_err": x0_err, "worst_ratio": post_err / 2e-5})
    torch.testing.assert_close(post.cpu(), s["post"], atol=2e-5, rtol=0)
    torch.testing.assert_close(x0d.cpu(), s["rec"], atol=2e-4, rtol=0)
    assert int((~sure).sum()) <= LOW_MARGIN_CAP
    assert not bool((mh & sure).any()) and not bool((mp & sure).any())


@gpu
@pytest.mark.parametrize("guided", [True, False], ids=["guided", "unguided"])
def test_step_kernel_three_waves_per_simd_equals_the_default(G, guided, monkeypatch):
    """GSDD_STEP_OCC=3 at K = 4096 runs d3pm_step_kernel<16, true, false, 3> (168-VGPR budget, scratch) instead of the production
    <16, true, false, 2>: the same tokens, token for token, and the oracle's wherever its margin exceeds 1e-3."""
    s = step_case(4096, guided)
    default, ok_d, _, _ = run_step(G, s, False)
    monkeypatch.setenv("GSDD_STEP_OCC", "3")
    occ3, ok_3, _, _ = run_step(G, s, False)
    sure = s["margin"] > 1e-3
    parity_report(f"objective_kernels::step_occ3[K4096_{'guided' if guided else 'unguided'}]",
                  {"low_margin": int((~sure).sum()), "differ_from_default": int((occ3 != default).sum()),
                   "mismatches": int((occ3 != s["tok"]).sum()), "worst_ratio": 0.0})
    assert ok_d and ok_3
    assert torch.equal(occ3, default)
    assert not bool(((occ3 != s["tok"]) & sure).any())


@gpu
@pytest.mark.parametrize("K", STEP_K)
def test_q_sample_at_every_class_width(G, K):
    """d3pm_q_sample against gumbel_argmax(q_pred(onehot(x0), t)): x0 = K, K - 1 and 0 among the tokens, t = T - 1 in the batch, 111
    positions, row0 = 1000, sentinels around x_t."""
    s = q_sample_case(K)
    sched = [s["sd"][n].cuda() for n in SCHED_ORDER]
    e = guarded((STEP_B, STEP_L), torch.int64, 16, 16)
    sid = torch.tensor([s["stream"]], dtype=torch.int64, device="cuda")
    G.ops.d3pm_q_sample(s["x0"].cuda(), e[1], sched, s["t"].cuda(), sid, K=K, T=T, seed=s["seed"], row0=STEP_ROW0)
    torch.cuda.synchronize()
    got = e[1].cpu()
    sure = s["margin"] > 1e-3
    mism = got != s["tok"]
    parity_report(f"objective_kernels::q_sample[K{K}]", {"positions": STEP_B * STEP_L, "low_margin": int((~sure).sum()),
                                                         "mismatches": int(mism.sum()), "worst_ratio": 0.0})
    assert intact(e), "d3pm_q_sample wrote outside x_t"
    assert int((~sure).sum()) <= LOW_MARGIN_CAP
    assert not bool((mism & sure).any())
