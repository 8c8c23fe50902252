// One SAC optimizer step as FOUR launches: critic gradients (+ the batch sum of the policy-gradient sample's "logprob"), critic
// apply (+ the temperature's Adam step), actor gradients, actor apply.
//
// replaces (reference, /root/reference/elegantrl/agent.py): AgentSAC.update_net's loop body (:442-468) -- get_obj_critic_raw
// (:519-527: minibatch gather, act.get_action_logprob(next_s) on the ONLINE actor (net.py:207-239), twin target heads + min + the
// entropy term, online twin forward, SmoothL1 x 2), obj_critic.backward(), cri_optimizer.step(), soft_update(cri_target) on every
// step (:116-124), act.get_action_logprob(state), obj_alpha and alpha_optimizer.step() (:452-458), alpha = exp(alpha_log),
// obj_actor = -(min(cri_target.get_q1_q2(state, a_pg)) + logprob * alpha).mean() (:461-463), obj_actor.backward(),
// act_optimizer.step().
//
// The decomposition is td3_fused.hip's (td3_device.hpp): a workgroup owns a 16-sample tile, its waves split every layer's output
// features, activations meet in LDS as chain images, md x md weights go global -> registers a layer ahead, every workgroup leaves a
// partial-gradient slab and td3_apply_kernel reduces the slabs in slab order, applies Adam and the soft update.  What SAC adds:
//   * the stochastic actor: ReLU, Hardswish, Hardswish body (the backward needs the Hardswish PRE-activations: they stay in
//     registers, the chain images hold the activations for the weight gradients), a mean and a log-std head, the re-parameterised
//     sample a = tanh(avg + exp(clamp(ls, -20, 2)) eps) and its "logprob" -- the reference's name for the NEGATIVE log-density
//     ls + log sqrt(2 pi) + eps^2 / 2 + log(1.000001 - a^2), used with that sign throughout.  (The reference writes the third term as
//     ((avg - u) / std)^2 / 2; its derivatives with respect to avg and std cancel, so nothing is propagated through it.)
//   * a grid-wide dependency in the middle of the step: the actor objective needs alpha AFTER the temperature's step, which needs the
//     batch mean of the policy-gradient sample's logprob.  The actor does not change between the critic launch and the temperature
//     step, so the critic launch -- which holds the gathered state rows and the actor's small tensors anyway -- also runs the actor
//     on `state` with the policy-gradient draws and leaves each workgroup's sum of logprob in word [1] of its slab's scalar slot;
//     the critic's apply launch, which reduces the slabs anyway, steps alpha_log (td3_apply_kernel, Td3ApplyArgs::temp); the actor
//     launch reads the new alpha_log and recomputes that forward, whose activations its backward needs anyway.  Cost: one extra
//     actor forward per sample (~66 k of ~550 k flop at width 128) instead of a fifth launch and a second pass over the batch.
//   * min(q1, q2) under the actor objective: both target heads are evaluated and the backward starts from each sample's own head.
// Draws: two tables of normals per step (parity tests inject the reference's) or Philox streams 4 (next-state sample) and 5
// (policy-gradient sample) in the kernels; both launches of a step form the same policy-gradient draw from (seed, epoch, row, position).
#include "sac.hpp"
#include "td3_device.hpp"

namespace pime {

constexpr uint32_t STREAM_SAC_NEXT = 4, STREAM_SAC_PG = 5;
constexpr float kLogSqrt2Pi = 0.91893853320467274178f;

// torch.nn.Hardswish: x relu6(x + 3) / 6; backward: 0 below -3, x / 3 + 0.5 up to and including 3, 1 above
__device__ __forceinline__ f32x4_t hsw4(f32x4_t v) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = v[r] * __builtin_amdgcn_fmed3f(v[r] + 3.0f, 0.f, 6.0f) * (1.0f / 6.0f);
    return v;
}
__device__ __forceinline__ f32x4_t hsg4(f32x4_t d, const f32x4_t& z) {
#pragma unroll
    for (int r = 0; r < 4; ++r) d[r] = z[r] < -3.0f ? 0.f : (z[r] <= 3.0f ? d[r] * (z[r] * (1.0f / 3.0f) + 0.5f) : d[r]);
    return d;
}

// the small tensors of ActorSAC (everything but the two md x md matrices) as one LDS image, in flat order (td3_device.hpp)
struct SacSmallActor { int W1, b1, b2, b3, wa, ba, ws, bs, total; };
__host__ __device__ inline SacSmallActor sac_small_actor(int D, int md) {
    const SacActorOff P = sac_actor_off(D, md);
    const int mm = md * md;
    return SacSmallActor{P.W1, P.b1, P.b2 - mm, P.b3 - 2 * mm, P.wa - 2 * mm, P.ba - 2 * mm, P.ws - 2 * mm, P.bs - 2 * mm, P.total - 2 * mm};
}
struct SacLds {
    int buf[4], xin, red, small[3], total;
};
__host__ __device__ inline SacLds sac_lds(int NT, int D) {
    SacLds L{};
    int o = 0;
    for (int k = 0; k < 4; ++k) { L.buf[k] = o; o += td3_buf_floats(NT); }
    L.xin = o; o += 16 * td3_xin_width(D);
    L.red = o; o += 8 * kRedSlot;
    const int md = NT * 16, sa = sac_small_actor(D, md).total, sc = td3_small_critic(D, md).total;
    L.small[0] = o; o += sa;                 // the online actor
    L.small[1] = o; o += sc;                 // critic launch: the online critic; actor launch: the target critic
    L.small[2] = o; o += sc;                 // critic launch only: the target critic
    L.total = o;
    return L;
}

__device__ __forceinline__ float sac_noise(const SacBatch& b, const float* table, uint32_t stream, long long trow, int pos) {
    if (table) return table[(size_t)trow * b.B + pos];
    const uint32_t epoch = b.noise_epoch + (b.epoch ? (uint32_t)b.epoch[0] : 0u);   // bumped by the host per update
    return philox_normal_f32(b.noise_seed, (uint32_t)pos, epoch, (uint32_t)trow, stream);
}

// net.py:207-239 for one sample, from the two heads' outputs and the draw
struct SacSample {
    float eps, std, a, corr, lp;
    bool open;   // the log-std clamp passes the gradient (-20 <= raw <= 2: torch's clamp backward includes both ends)
};
__device__ __forceinline__ SacSample sac_sample(float avg, float raw, float eps) {
    SacSample s;
    const float ls = fminf(fmaxf(raw, -20.0f), 2.0f);
    s.eps = eps;
    s.open = raw >= -20.0f && raw <= 2.0f;
    s.std = expf(ls);
    s.a = tanhf(avg + s.std * eps);
    s.corr = 1.000001f - s.a * s.a;
    s.lp = ls + kLogSqrt2Pi + 0.5f * eps * eps + logf(s.corr);
    return s;
}

// ActorSAC's body and heads on this tile's rows (x: the lane's first-layer B operands).  wA holds net_state.2's weights on entry;
// net_state.4's are loaded into wB here (LOADB) or still stand there from an earlier call; NEXTA: weights to load into wA once
// net_state.2 is done with it.  Leaves h1 = relu(z1) in B0 and hardswish(z2) in B1 (the operands of the weight gradients), the
// pre-activations z2, z3 in registers, and every lane's sample's head outputs.  Ends behind a barrier.
template <int NT, int PER, int NW, int KF, bool LOADB>
__device__ __forceinline__ void sac_actor_fwd(const float* __restrict__ actg, const SacActorOff& PA, const float* __restrict__ ac,
                                              const SacSmallActor& SA, int D, float* __restrict__ B0, float* __restrict__ B1,
                                              float* __restrict__ red, int slot, int wave, int t0, int lane, const float (&x)[KF],
                                              Wts<NT, PER, false>& wA, Wts<NT, PER, false>& wB, const float* __restrict__ nextA,
                                              f32x4_t (&in)[NT], f32x4_t (&h1)[PER], f32x4_t (&z2)[PER], f32x4_t (&z3)[PER],
                                              float& avg, float& raw) {
    layer_first<PER, KF>(ac + SA.W1, ac + SA.b1, D, t0, lane, x, h1);
#pragma unroll
    for (int n = 0; n < PER; ++n) { h1[n] = relu4(h1[n]); chain_put(B0, lane, t0 + n, h1[n]); }
    if (LOADB) wload(wB, actg + PA.W3, t0, lane);
    bias_get<PER>(ac + SA.b2, t0, lane, z2);   // a layer's accumulators start as its bias, read in front of the barrier
    TD3_BARRIER();
    chain_get<NT>(B0, lane, in);
    wlayer(wA, in, z2);
#pragma unroll
    for (int n = 0; n < PER; ++n) chain_put(B1, lane, t0 + n, hsw4(z2[n]));
    if (nextA) wload(wA, nextA, t0, lane);
    bias_get<PER>(ac + SA.b3, t0, lane, z3);
    TD3_BARRIER();
    chain_get<NT>(B1, lane, in);
    wlayer(wB, in, z3);
    f32x4_t h3[PER];
#pragma unroll
    for (int n = 0; n < PER; ++n) h3[n] = hsw4(z3[n]);
    red_put(red, slot, wave, lane, head_partial<PER>(ac + SA.wa, t0, lane, h3));
    red_put(red, slot + 1, wave, lane, head_partial<PER>(ac + SA.ws, t0, lane, h3));
    TD3_BARRIER();
    avg = red_get<NW>(red, slot, lane) + ac[SA.ba];
    raw = red_get<NW>(red, slot + 1, lane) + ac[SA.bs];
}

// ======================================================================================================== critic gradients
// DD: the state width as a compile-time constant (3: pH, 4: water tank Integrator), 0: read from the arguments (td3_fused.hip).
template <int MD, int DD, int NW>
__global__ __launch_bounds__(NW * 64, 1) void sac_critic_kernel(SacGradArgs a) {
    constexpr int NT = MD / 16, PER = NT / NW, KF = 2, XW = 16, XG = 4 * KF;
    static_assert(PER >= 1 && PER * NW == NT, "the waves split a layer's output tiles evenly");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int D = DD ? DD : a.D, Dc = D + 1;
    const SacLds F = sac_lds(NT, D);
    float* const B0 = lds + F.buf[0];
    float* const B1 = lds + F.buf[1];
    float* const B2 = lds + F.buf[2];
    float* const xin = lds + F.xin;
    float* const red = lds + F.red;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t0 = wave * PER;
    const SacActorOff PA = sac_actor_off(D, MD);
    const Td3CriticOff PC = td3_critic_off(D, MD);
    const SacSmallActor SA = sac_small_actor(D, MD);
    const Td3SmallCritic SC = td3_small_critic(D, MD);
    const float* const ac = lds + F.small[0];   // online actor, small tensors
    const float* const cr = lds + F.small[1];   // online critic
    const float* const ct = lds + F.small[2];   // target critic
    const Td3SlabLayout SL = td3_critic_slab(D, MD);
    const float invB = 1.0f / (float)a.b.B;
    const float alpha = expf(a.alpha_log[0]);   // as the previous step's temperature update left it (agent.py:436,461)
    const long long trow = a.b.row;
    float* const sl = a.slab + (size_t)blockIdx.x * a.stride;
    float loss_acc = 0.f, lp_acc = 0.f;   // wave 0, lanes 0..15: this workgroup's loss terms / logprob of the policy-gradient sample

#pragma unroll 1
    for (int group = blockIdx.x; group < a.ngroups; group += gridDim.x) {
        int lane = tid & 63;
        asm volatile("" : "+v"(lane));
        const int j = lane & 15, q = lane >> 4;
        const bool accum = group != (int)blockIdx.x;
        const int pos = group * kTd3Tile + j;
        const bool valid = pos < a.b.B;
        const int p = valid ? pos : a.b.B - 1;
        const long long row = a.b.idx[(size_t)trow * a.b.B + p], nrow = a.b.nxt[(size_t)trow * a.b.B + p];
        Wts<NT, PER, false> wA, wB;
        f32x4_t in[NT];
        wload(wA, a.act + PA.W2, t0, lane);   // the first md x md weights: in flight behind the gather's two round trips
        if (!accum) {   // the nets' small tensors (first group only)
            small_copy<NW * 64>(lds + F.small[0], a.act, PA.W1, PA.W2, tid);
            small_copy<NW * 64>(lds + F.small[0] + SA.b2, a.act, PA.b2, PA.W3, tid);
            small_copy<NW * 64>(lds + F.small[0] + SA.b3, a.act, PA.b3, PA.total, tid);
            small_copy<NW * 64>(lds + F.small[1], a.cri, PC.W1, PC.W2, tid);
            small_copy<NW * 64>(lds + F.small[1] + SC.b2, a.cri, PC.b2, PC.total, tid);
            small_copy<NW * 64>(lds + F.small[2], a.cri_target, PC.W1, PC.W2, tid);
            small_copy<NW * 64>(lds + F.small[2] + SC.b2, a.cri_target, PC.b2, PC.total, tid);
        }
        // first-layer B operands: input column 4 k + q of sample j
        const float* srow = a.b.state + (size_t)row * D;
        const float* nsrow = a.b.state + (size_t)nrow * D;
        float sx[KF], nx[KF];
#pragma unroll
        for (int k = 0; k < KF; ++k) {
            sx[k] = 4 * k + q < D ? srow[4 * k + q] : 0.f;
            nx[k] = 4 * k + q < D ? nsrow[4 * k + q] : 0.f;
        }
        const float* orow = a.b.other + (size_t)row * 3;
        const float reward = orow[0], mask = orow[1], action = orow[2];
        const float eps_next = sac_noise(a.b, a.b.noise_next, STREAM_SAC_NEXT, trow, p);
        const float eps_pg = sac_noise(a.b, a.b.noise_pg, STREAM_SAC_PG, trow, p);
        TD3_BARRIER();   // the previous group is done with the LDS images; the small tensors are in
        // the online critic's input [s, a, 0 ..]: column 4 k + q of sample j (this lane's first-layer B operands)
        float xs[KF];
#pragma unroll
        for (int k = 0; k < KF; ++k) xs[k] = 4 * k + q < D ? sx[k] : (4 * k + q == D ? action : 0.f);
        if (wave == 0) {   // ... as rows [16 samples][XW columns] for its first-layer weight gradient, and for the actor launch
#pragma unroll
            for (int k = 0; k < XW / 4; ++k) xin[j * XW + 4 * k + q] = k < KF ? xs[k] : 0.f;
            if (valid) {
#pragma unroll
                for (int k = 0; k < KF; ++k) a.xg[(size_t)pos * XG + 4 * k + q] = xs[k];
            }
        }

        // ------------------------------------------------------------------ next_a, next_lp = act.get_action_logprob(s')
        float next_a, next_lp;
        {
            f32x4_t h1[PER], z2[PER], z3[PER];
            float avg, raw;
            sac_actor_fwd<NT, PER, NW, KF, true>(a.act, PA, ac, SA, D, B0, B1, red, 0, wave, t0, lane, nx, wA, wB, nullptr, in, h1, z2, z3, avg, raw);
            const SacSample s = sac_sample(avg, raw, eps_next);
            next_a = s.a;
            next_lp = s.lp;
            // ---------------------------------------------------------------- lp of a_pg = act.get_action_logprob(s): the temperature's gradient
            sac_actor_fwd<NT, PER, NW, KF, false>(a.act, PA, ac, SA, D, B0, B1, red, 2, wave, t0, lane, sx, wA, wB, a.cri_target + PC.W2, in, h1, z2,
                                                  z3, avg, raw);
            const SacSample g = sac_sample(avg, raw, eps_pg);
            if (valid && wave == 0 && q == 0) lp_acc += g.lp;
        }
        // ------------------------------------------------------------------ q_label = r + mask * (min(cri_target twin heads)(s', next_a) + next_lp alpha)
        wload(wB, a.cri + PC.W2, t0, lane);
        float label;
        {
            float xt[KF];
#pragma unroll
            for (int k = 0; k < KF; ++k) xt[k] = 4 * k + q < D ? nx[k] : (4 * k + q == D ? next_a : 0.f);
            f32x4_t h[PER];
            layer_first<PER, KF>(ct + SC.W1, ct + SC.b1, Dc, t0, lane, xt, h);
#pragma unroll
            for (int n = 0; n < PER; ++n) chain_put(B0, lane, t0 + n, relu4(h[n]));
            bias_get<PER>(ct + SC.b2, t0, lane, h);
            TD3_BARRIER();
            chain_get<NT>(B0, lane, in);
            wlayer(wA, in, h);
#pragma unroll
            for (int n = 0; n < PER; ++n) h[n] = relu4(h[n]);
            red_put(red, 4, wave, lane, head_partial<PER>(ct + SC.q1w, t0, lane, h));
            red_put(red, 5, wave, lane, head_partial<PER>(ct + SC.q2w, t0, lane, h));
            TD3_BARRIER();
            const float tq1 = red_get<NW>(red, 4, lane) + ct[SC.q1b], tq2 = red_get<NW>(red, 5, lane) + ct[SC.q2b];
            label = reward + mask * (fminf(tq1, tq2) + next_lp * alpha);
        }
        // ------------------------------------------------------------------ online twin critic on (s, a): forward
        f32x4_t h1[PER], h2[PER];
        {
            layer_first<PER, KF>(cr + SC.W1, cr + SC.b1, Dc, t0, lane, xs, h1);
#pragma unroll
            for (int n = 0; n < PER; ++n) { h1[n] = relu4(h1[n]); chain_put(B1, lane, t0 + n, h1[n]); }
        }
        wload_t(wA, a.cri + PC.W2, t0, lane);   // for dH1 = W2^T dZ2
        bias_get<PER>(cr + SC.b2, t0, lane, h2);
        TD3_BARRIER();
        chain_get<NT>(B1, lane, in);
        wlayer(wB, in, h2);
#pragma unroll
        for (int n = 0; n < PER; ++n) h2[n] = relu4(h2[n]);
        red_put(red, 6, wave, lane, head_partial<PER>(cr + SC.q1w, t0, lane, h2));
        red_put(red, 7, wave, lane, head_partial<PER>(cr + SC.q2w, t0, lane, h2));
        TD3_BARRIER();
        // ------------------------------------------------------------------ SmoothL1 x 2 (beta = 1, mean) and its gradient
        float g1 = 0.f, g2 = 0.f;
        {
            const float d1 = red_get<NW>(red, 6, lane) + cr[SC.q1b] - label, d2 = red_get<NW>(red, 7, lane) + cr[SC.q2b] - label;
            const float a1 = fabsf(d1), a2 = fabsf(d2);
            if (valid) {
                g1 = (a1 < 1.f ? d1 : (d1 > 0.f ? 1.f : -1.f)) * invB;
                g2 = (a2 < 1.f ? d2 : (d2 > 0.f ? 1.f : -1.f)) * invB;
                if (wave == 0 && q == 0) loss_acc += (a1 < 1.f ? 0.5f * d1 * d1 : a1 - 0.5f) + (a2 < 1.f ? 0.5f * d2 * d2 : a2 - 0.5f);
            }
        }
        // heads: weight / bias gradients, dZ2 = (g1 wq1 + g2 wq2) [h2 > 0]
        {
            f32x4_t v1[PER], v2[PER], dz[PER];
#pragma unroll
            for (int n = 0; n < PER; ++n) {
                const f32x4_t w1 = ld4(cr + SC.q1w + 16 * (t0 + n) + 4 * q), w2 = ld4(cr + SC.q2w + 16 * (t0 + n) + 4 * q);
                v1[n] = h2[n] * g1;
                v2[n] = h2[n] * g2;
                dz[n] = gate4(w1 * g1 + w2 * g2, h2[n]);
                chain_put(B2, lane, t0 + n, dz[n]);
            }
            vec_grad<PER>(sl + SL.seg[4].slab_off, t0, lane, v1, accum);
            vec_grad<PER>(sl + SL.seg[6].slab_off, t0, lane, v2, accum);
            vec_grad<PER>(sl + SL.seg[3].slab_off, t0, lane, dz, accum);   // net_sa.2 bias
            if (wave == 0) {
                const float b1 = row_sum16(g1), b2 = row_sum16(g2);
                if (lane == 0) {
                    float* p1 = sl + SL.seg[5].slab_off;
                    float* p2 = sl + SL.seg[7].slab_off;
                    p1[0] = accum ? p1[0] + b1 : b1;
                    p2[0] = accum ? p2[0] + b2 : b2;
                }
            }
        }
        TD3_BARRIER();   // dZ2 published
        dw_slab<NT, PER, false>(B2, B1, sl + SL.seg[2].slab_off, t0, lane, accum);   // net_sa.2 weight gradient
        TD3_NO_HOIST();
        chain_get<NT>(B2, lane, in);
        {
            f32x4_t d1[PER];
            zero4<PER>(d1);
            wlayer(wA, in, d1);
#pragma unroll
            for (int n = 0; n < PER; ++n) { d1[n] = gate4(d1[n], h1[n]); chain_put(B0, lane, t0 + n, d1[n]); }
            vec_grad<PER>(sl + SL.seg[1].slab_off, t0, lane, d1, accum);   // net_sa.0 bias
        }
        TD3_BARRIER();   // dZ1 published
        {
            f32x4_t acc[PER][1];
            dw_first<PER, XW>(B0, xin, t0, lane, acc);
            float* seg = sl + SL.seg[0].slab_off;
#pragma unroll
            for (int n = 0; n < PER; ++n) slab_put(seg + ((t0 + n) * 64 + lane) * 4, acc[n][0], accum);
        }
    }
    if (wave == 0) {
        const float t = row_sum16(loss_acc), l = row_sum16(lp_acc);
        if (tid == 0) st4(sl + SL.scalar_off, f32x4_t{t, l, 0.f, 0.f});
    }
}

// ======================================================================================================== actor gradients
// obj_actor = -mean(min(cri_target.get_q1_q2(s, a_pg)) + lp alpha)  (agent.py:461-463), differentiated down to the actor's parameters
template <int MD, int DD, int NW>
__global__ __launch_bounds__(NW * 64, 1) void sac_actor_kernel(SacGradArgs a) {
    constexpr int NT = MD / 16, PER = NT / NW, KF = 2, XW = 16, XG = 4 * KF;
    static_assert(PER >= 1 && PER * NW == NT, "the waves split a layer's output tiles evenly");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int D = DD ? DD : a.D, Dc = D + 1;
    const SacLds F = sac_lds(NT, D);
    float* const B0 = lds + F.buf[0];
    float* const B1 = lds + F.buf[1];
    float* const B2 = lds + F.buf[2];
    float* const B3 = lds + F.buf[3];
    float* const xin = lds + F.xin;
    float* const red = lds + F.red;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t0 = wave * PER;
    const SacActorOff PA = sac_actor_off(D, MD);
    const Td3CriticOff PC = td3_critic_off(D, MD);
    const SacSmallActor SA = sac_small_actor(D, MD);
    const Td3SmallCritic SC = td3_small_critic(D, MD);
    const float* const ac = lds + F.small[0];   // online actor, small tensors
    const float* const ct = lds + F.small[1];   // target critic, as this step's soft update left it
    const Td3SlabLayout SL = sac_actor_slab(D, MD);
    const float invB = 1.0f / (float)a.b.B;
    const float alpha = expf(a.alpha_log[0]);   // after this step's temperature update (agent.py:461)
    const long long trow = a.b.row;
    float* const sl = a.slab + (size_t)blockIdx.x * a.stride;
    float q_acc = 0.f;

#pragma unroll 1
    for (int group = blockIdx.x; group < a.ngroups; group += gridDim.x) {
        int lane = tid & 63;
        asm volatile("" : "+v"(lane));
        const int j = lane & 15, q = lane >> 4;
        const bool accum = group != (int)blockIdx.x;
        const int pos = group * kTd3Tile + j;
        const bool valid = pos < a.b.B;
        const int p = valid ? pos : a.b.B - 1;
        Wts<NT, PER, false> wA, wB;
        f32x4_t in[NT];
        wload(wA, a.act + PA.W2, t0, lane);
        // the minibatch's state rows as the critic launch of this step gathered them (one round trip instead of index -> row)
        float sx[KF];
#pragma unroll
        for (int k = 0; k < KF; ++k) sx[k] = 4 * k + q < D ? a.xg[(size_t)p * XG + 4 * k + q] : 0.f;
        const float eps_pg = sac_noise(a.b, a.b.noise_pg, STREAM_SAC_PG, trow, p);
        if (!accum) {   // the small tensors (first group only)
            small_copy<NW * 64>(lds + F.small[0], a.act, PA.W1, PA.W2, tid);
            small_copy<NW * 64>(lds + F.small[0] + SA.b2, a.act, PA.b2, PA.W3, tid);
            small_copy<NW * 64>(lds + F.small[0] + SA.b3, a.act, PA.b3, PA.total, tid);
            small_copy<NW * 64>(lds + F.small[1], a.cri, PC.W1, PC.W2, tid);
            small_copy<NW * 64>(lds + F.small[1] + SC.b2, a.cri, PC.b2, PC.total, tid);
        }
        TD3_BARRIER();   // the previous group is done with the LDS images; the small tensors are in
        if (wave == 0) {   // the actor's input rows [16 samples][XW columns, zero beyond D] for its first-layer weight gradient
#pragma unroll
            for (int k = 0; k < XW / 4; ++k) xin[j * XW + 4 * k + q] = k < KF ? sx[k] : 0.f;
        }
        f32x4_t a1[PER], z2[PER], z3[PER], c1[PER], c2[PER];

        // ------------------------------------------------------------------ a_pg, lp = act.get_action_logprob(s): h1 in B0, h2 in B1
        float avg, raw;
        sac_actor_fwd<NT, PER, NW, KF, true>(a.act, PA, ac, SA, D, B0, B1, red, 0, wave, t0, lane, sx, wA, wB, a.cri + PC.W2, in, a1, z2, z3, avg, raw);
        const SacSample s = sac_sample(avg, raw, eps_pg);
        // ------------------------------------------------------------------ q1, q2 = cri_target.get_q1_q2(s, a_pg)
        {
            float xt[KF];
#pragma unroll
            for (int k = 0; k < KF; ++k) xt[k] = 4 * k + q < D ? sx[k] : (4 * k + q == D ? s.a : 0.f);
            layer_first<PER, KF>(ct + SC.W1, ct + SC.b1, Dc, t0, lane, xt, c1);
#pragma unroll
            for (int n = 0; n < PER; ++n) { c1[n] = relu4(c1[n]); chain_put(B2, lane, t0 + n, c1[n]); }
        }
        wload_t(wB, a.cri + PC.W2, t0, lane);   // dC1 = W2^T dZc2
        bias_get<PER>(ct + SC.b2, t0, lane, c2);
        TD3_BARRIER();
        chain_get<NT>(B2, lane, in);
        wlayer(wA, in, c2);
#pragma unroll
        for (int n = 0; n < PER; ++n) c2[n] = relu4(c2[n]);
        red_put(red, 2, wave, lane, head_partial<PER>(ct + SC.q1w, t0, lane, c2));
        red_put(red, 3, wave, lane, head_partial<PER>(ct + SC.q2w, t0, lane, c2));
        wload_t(wA, a.act + PA.W3, t0, lane);   // dA2 = W3^T dZ3
        TD3_BARRIER();
        // ------------------------------------------------------------------ backward through the critic to the action, from each sample's own head
        const float g = valid ? -invB : 0.f;   // d obj / d (min q + lp alpha)
        {
            const float q1 = red_get<NW>(red, 2, lane) + ct[SC.q1b], q2 = red_get<NW>(red, 3, lane) + ct[SC.q2b];
            const bool first = q1 <= q2;
            if (valid && wave == 0 && q == 0) q_acc += (first ? q1 : q2) + s.lp * alpha;
#pragma unroll
            for (int n = 0; n < PER; ++n) {
                const f32x4_t w1 = ld4(ct + SC.q1w + 16 * (t0 + n) + 4 * q), w2 = ld4(ct + SC.q2w + 16 * (t0 + n) + 4 * q);
                chain_put(B3, lane, t0 + n, gate4((first ? w1 : w2) * g, c2[n]));
            }
        }
        TD3_BARRIER();
        chain_get<NT>(B3, lane, in);
        float g_u, g_raw;
        {
            f32x4_t d[PER];
            zero4<PER>(d);
            wlayer(wB, in, d);
            float pa = 0.f;   // d obj / d action through the critic = sum_f W1[f][D] dZc1[f]
#pragma unroll
            for (int n = 0; n < PER; ++n) {
                d[n] = gate4(d[n], c1[n]);
#pragma unroll
                for (int r = 0; r < 4; ++r) pa = fmaf(d[n][r], ct[SC.W1 + (16 * (t0 + n) + 4 * q + r) * Dc + D], pa);
            }
            pa += __shfl_xor(pa, 16);
            pa += __shfl_xor(pa, 32);
            red_put(red, 4, wave, lane, pa);
            TD3_BARRIER();
            const float g_lp = g * alpha;                                             // d obj / d lp
            const float g_a = red_get<NW>(red, 4, lane) + g_lp * (-2.0f * s.a / s.corr);   // + the tanh correction log(1.000001 - a^2)
            g_u = g_a * (1.0f - s.a * s.a);                                           // tanh'; d u / d avg = 1
            g_raw = s.open ? g_u * s.std * s.eps + g_lp : 0.f;                        // u = avg + exp(ls) eps, lp = ls + ...; the clamp's gate
        }
        // ------------------------------------------------------------------ actor backward + weight gradients
        {
            f32x4_t va[PER], vs[PER], dz[PER];
#pragma unroll
            for (int n = 0; n < PER; ++n) {
                const f32x4_t wa = ld4(ac + SA.wa + 16 * (t0 + n) + 4 * q), ws = ld4(ac + SA.ws + 16 * (t0 + n) + 4 * q);
                const f32x4_t h3 = hsw4(z3[n]);
                va[n] = h3 * g_u;
                vs[n] = h3 * g_raw;
                dz[n] = hsg4(wa * g_u + ws * g_raw, z3[n]);
                chain_put(B2, lane, t0 + n, dz[n]);
            }
            vec_grad<PER>(sl + SL.seg[6].slab_off, t0, lane, va, accum);   // net_a_avg weight
            vec_grad<PER>(sl + SL.seg[8].slab_off, t0, lane, vs, accum);   // net_a_std weight
            vec_grad<PER>(sl + SL.seg[5].slab_off, t0, lane, dz, accum);   // net_state.4 bias
            if (wave == 0) {
                const float ba = row_sum16(g_u), bs = row_sum16(g_raw);
                if (lane == 0) {
                    float* pa = sl + SL.seg[7].slab_off;
                    float* ps = sl + SL.seg[9].slab_off;
                    pa[0] = accum ? pa[0] + ba : ba;
                    ps[0] = accum ? ps[0] + bs : bs;
                }
            }
        }
        wload_t(wB, a.act + PA.W2, t0, lane);   // dA1 = W2^T dZ2
        TD3_BARRIER();   // dZ3 published
        dw_slab<NT, PER, false>(B2, B1, sl + SL.seg[4].slab_off, t0, lane, accum);   // net_state.4: dZ3^T H2
        TD3_NO_HOIST();
        chain_get<NT>(B2, lane, in);
        {
            f32x4_t d[PER];
            zero4<PER>(d);
            wlayer(wA, in, d);
#pragma unroll
            for (int n = 0; n < PER; ++n) { d[n] = hsg4(d[n], z2[n]); chain_put(B3, lane, t0 + n, d[n]); }
            vec_grad<PER>(sl + SL.seg[3].slab_off, t0, lane, d, accum);    // net_state.2 bias
        }
        TD3_BARRIER();   // dZ2 published
        dw_slab<NT, PER, false>(B3, B0, sl + SL.seg[2].slab_off, t0, lane, accum);   // net_state.2: dZ2^T H1
        TD3_NO_HOIST();
        chain_get<NT>(B3, lane, in);
        {
            f32x4_t d[PER];
            zero4<PER>(d);
            wlayer(wB, in, d);
#pragma unroll
            for (int n = 0; n < PER; ++n) { d[n] = gate4(d[n], a1[n]); chain_put(B1, lane, t0 + n, d[n]); }
            vec_grad<PER>(sl + SL.seg[1].slab_off, t0, lane, d, accum);    // net_state.0 bias
        }
        TD3_BARRIER();   // dZ1 published
        {
            f32x4_t acc[PER][1];
            dw_first<PER, XW>(B1, xin, t0, lane, acc);
            float* seg = sl + SL.seg[0].slab_off;
#pragma unroll
            for (int n = 0; n < PER; ++n) slab_put(seg + ((t0 + n) * 64 + lane) * 4, acc[n][0], accum);
        }
    }
    if (wave == 0) {
        const float t = row_sum16(q_acc);
        if (tid == 0) st4(sl + SL.scalar_off, f32x4_t{t, 0.f, 0.f, 0.f});
    }
}

// ======================================================================================================== host side
bool sac_supported(int D, int A, int md) { return A == 1 && D >= 1 && D <= kSacMaxD && (md == 64 || md == 128); }
int64_t sac_workspace_floats(int D, int md, int B) {
    const int64_t g = td3_grid(B);
    // slabs + the gathered rows [B][td3_xg_stride(D)]
    return g * (sac_actor_slab(D, md).stride + td3_critic_slab(D, md).stride) + (int64_t)B * td3_xg_stride(D);
}

// waves per workgroup as for TD3: four at width 64 (one per SIMD), eight at width 128
template <int MD, int DD>
static int launch_grad_d(bool critic, const SacGradArgs& a, int grid, hipStream_t s) {
    constexpr int NW = MD == 64 ? 4 : 8;
    const size_t lds_bytes = sizeof(float) * (size_t)sac_lds(MD / 16, a.D).total;
    if (critic) hipLaunchKernelGGL((sac_critic_kernel<MD, DD, NW>), dim3(grid), dim3(NW * 64), lds_bytes, s, a);
    else hipLaunchKernelGGL((sac_actor_kernel<MD, DD, NW>), dim3(grid), dim3(NW * 64), lds_bytes, s, a);
    PIME_HIP_TRY(hipGetLastError());
    return PIME_OK;
}
template <int MD>
static int launch_grad(bool critic, const SacGradArgs& a, int grid, hipStream_t s) {
    if (a.D == 3) return launch_grad_d<MD, 3>(critic, a, grid, s);   // pH observation
    if (a.D == 4) return launch_grad_d<MD, 4>(critic, a, grid, s);   // water-tank Integrator observation
    return launch_grad_d<MD, 0>(critic, a, grid, s);
}
int launch_sac_grad(bool critic, int md, const SacGradArgs& a, int grid, hipStream_t s) {
    if (!sac_supported(a.D, 1, md)) {
        set_error("no fused SAC instantiation for state_dim %d width %d", a.D, md);
        return PIME_ERR_ARG;
    }
    return md == 128 ? launch_grad<128>(critic, a, grid, s) : launch_grad<64>(critic, a, grid, s);
}

}  // namespace pime
