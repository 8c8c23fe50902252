// One SAC optimizer step as FOUR launches: critic gradients (+ the batch sum of the policy-gradient sample's "logprob"), critic
// apply (+ the temperature's Adam step), actor gradients, actor apply.
//
// replaces (reference, elegantrl/agent.py): AgentSAC.update_net's loop body (:442-468) -- get_obj_critic_raw
// (:519-527: minibatch gather, act.get_action_logprob(next_s) on the ONLINE actor (net.py:207-239), twin target heads + min + the
// entropy term, online twin forward, SmoothL1 x 2), obj_critic.backward(), cri_optimizer.step(), soft_update(cri_target) on every
// step (:116-124), act.get_action_logprob(state), obj_alpha and alpha_optimizer.step() (:452-458), alpha = exp(alpha_log),
// obj_actor = -(min(cri_target.get_q1_q2(state, a_pg)) + logprob * alpha).mean() (:461-463), obj_actor.backward(),
// act_optimizer.step().
//
// The decomposition is the TD3 step's (td3_fused.hip's header describes it), and so is most of the device code: the tile context, the
// gather, the twin target heads, the online twin-critic step, the target critic's forward and backward to the action, the actor
// body's backward and the launch dispatch are the shared pieces of td3_device.hpp; the apply launches are td3_apply_kernel.  What is
// this file's own:
//   * the stochastic actor (sac_actor_fwd): ReLU, Hardswish, Hardswish body (the backward needs the Hardswish PRE-activations: they
//     stay in registers, the chain images hold the activations for the weight gradients), a mean and a log-std head, the
//     re-parameterised sample a = tanh(avg + exp(clamp(ls, -20, 2)) eps) and its "logprob" -- the reference's name for the NEGATIVE
//     log-density ls + log sqrt(2 pi) + eps^2 / 2 + log(1.000001 - a^2), used with that sign throughout.  (The reference writes the
//     third term as ((avg - u) / std)^2 / 2; its derivatives with respect to avg and std cancel, so nothing is propagated through it.)
//   * a grid-wide dependency in the middle of the step: the actor objective needs alpha AFTER the temperature's step, which needs the
//     batch mean of the policy-gradient sample's logprob.  The actor does not change between the critic launch and the temperature
//     step, so the critic launch -- which holds the gathered state rows and the actor's small tensors anyway -- also runs the actor
//     on `state` with the policy-gradient draws and leaves each workgroup's sum of logprob in word [1] of its slab's scalar slot;
//     the critic's apply launch, which reduces the slabs anyway, steps alpha_log (td3_apply_kernel, Td3ApplyArgs::temp); the actor
//     launch reads the new alpha_log and recomputes that forward, whose activations its backward needs anyway.  Cost: one extra
//     actor forward per sample (~66 k of ~550 k flop at width 128) instead of a fifth launch and a second pass over the batch.
//   * the entropy term of the label, and min(q1, q2) under the actor objective: both target heads are evaluated and the backward
//     starts from each sample's own head; the two heads' gradients and the Hardswish gates of the actor's backward.
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
struct GateHardswish {   // actor_body_bwd's gate (td3_device.hpp), on the stored pre-activations
    static __device__ __forceinline__ f32x4_t bwd(const f32x4_t& d, const f32x4_t& z) { return hsg4(d, z); }
};

// the small tensors of ActorSAC (everything but the two md x md matrices) as one LDS image, in flat order (td3_device.hpp)
struct SacSmallActor { int W1, b1, b2, b3, wa, ba, ws, bs, total; };
__host__ __device__ inline SacSmallActor sac_small_actor(int D, int md) {
    const SacActorOff P = sac_actor_off(D, md);
    const int mm = md * md;
    return SacSmallActor{P.W1, P.b1, P.b2 - mm, P.b3 - 2 * mm, P.wa - 2 * mm, P.ba - 2 * mm, P.ws - 2 * mm, P.bs - 2 * mm, P.total - 2 * mm};
}
// TD3's LDS map around ActorSAC's small image (small[0]: the online actor, in both launches)
__host__ __device__ inline Td3Lds sac_lds(int NT, int D) { return td3_lds(NT, D, sac_small_actor(D, NT * 16).total); }

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
    constexpr int NT = MD / 16, PER = NT / NW, KF = 2, XW = 16;
    constexpr bool S = false;   // register-resident md x md weights (width <= 128)
    static_assert(PER >= 1 && PER * NW == NT, "the waves split a layer's output tiles evenly");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int D = DD ? DD : a.D, Dc = D + 1;
    const Td3Lds F = sac_lds(NT, D);
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
        const Td3Tile T = td3_tile(tid, group, a.b.B);
        const int lane = T.lane;
        Td3Gather<KF> G;
        gather_index(G, a.b, T);
        Wts<NT, PER, S> wA, wB;
        f32x4_t in[NT];
        wload(wA, a.act + PA.W2, t0, lane);   // the first md x md weights: in flight behind the gather's two round trips
        if (!T.accum) {   // the nets' small tensors (first group only)
            small_copy_actor<NW * 64>(lds + F.small[0], a.act, PA.W1, PA, SA, tid);
            small_copy_critic<NW * 64>(lds + F.small[1], a.cri, PC.W1, PC, SC, tid);
            small_copy_critic<NW * 64>(lds + F.small[2], a.cri_target, PC.W1, PC, SC, tid);
        }
        gather_rows(G, a.b, D, T);
        const float eps_next = sac_noise(a.b, a.b.noise_next, STREAM_SAC_NEXT, trow, T.p);
        const float eps_pg = sac_noise(a.b, a.b.noise_pg, STREAM_SAC_PG, trow, T.p);
        TD3_BARRIER();   // the previous group is done with the LDS images; the small tensors are in
        gather_publish<KF, XW>(G, D, T, wave, xin, a.xg);

        // ------------------------------------------------------------------ next_a, next_lp = act.get_action_logprob(s')
        float next_a, next_lp;
        {
            f32x4_t h1[PER], z2[PER], z3[PER];
            float avg, raw;
            sac_actor_fwd<NT, PER, NW, KF, true>(a.act, PA, ac, SA, D, B0, B1, red, 0, wave, t0, lane, G.nx, wA, wB, nullptr, in, h1, z2, z3, avg, raw);
            const SacSample s = sac_sample(avg, raw, eps_next);
            next_a = s.a;
            next_lp = s.lp;
            // ---------------------------------------------------------------- lp of a_pg = act.get_action_logprob(s): the temperature's gradient
            sac_actor_fwd<NT, PER, NW, KF, false>(a.act, PA, ac, SA, D, B0, B1, red, 2, wave, t0, lane, G.sx, wA, wB, a.cri_target + PC.W2, in, h1,
                                                  z2, z3, avg, raw);
            const SacSample g = sac_sample(avg, raw, eps_pg);
            if (T.valid && wave == 0 && T.q == 0) lp_acc += g.lp;
        }
        // ------------------------------------------------------------------ q_label = r + mask * (min(cri_target twin heads)(s', next_a) + next_lp alpha)
        wload(wB, a.cri + PC.W2, t0, lane);
        float xt[KF], tq1, tq2;
        critic_input<KF>(G.nx, next_a, D, T.q, xt);
        twin_heads<NT, PER, NW, KF, S>(ct + SC.W1, ct, SC, Dc, B0, red, 4, wave, t0, lane, xt, wA, in, tq1, tq2);
        const float label = G.reward + G.mask * (fminf(tq1, tq2) + next_lp * alpha);
        // ------------------------------------------------------------------ online twin critic on (s, a): loss, backward, weight gradients
        online_critic_step<NT, PER, NW, KF, XW, S>(cr + SC.W1, cr, SC, a.cri + PC.W2, Dc, B0, B1, B2, xin, red, 6, wave, t0, T, G.xs, label, invB,
                                                   wA, wB, in, sl, SL, loss_acc);
    }
    tile_scalars_put(sl + SL.scalar_off, wave, tid, {loss_acc, lp_acc});
}

// ======================================================================================================== actor gradients
// obj_actor = -mean(min(cri_target.get_q1_q2(s, a_pg)) + lp alpha)  (agent.py:461-463), differentiated down to the actor's parameters
template <int MD, int DD, int NW>
__global__ __launch_bounds__(NW * 64, 1) void sac_actor_kernel(SacGradArgs a) {
    constexpr int NT = MD / 16, PER = NT / NW, KF = 2, XW = 16;
    constexpr bool S = false;   // register-resident md x md weights (width <= 128)
    static_assert(PER >= 1 && PER * NW == NT, "the waves split a layer's output tiles evenly");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int D = DD ? DD : a.D, Dc = D + 1;
    const Td3Lds F = sac_lds(NT, D);
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
        const Td3Tile T = td3_tile(tid, group, a.b.B);
        const int lane = T.lane, q = T.q;
        const bool accum = T.accum;
        Wts<NT, PER, S> wA, wB;
        f32x4_t in[NT];
        wload(wA, a.act + PA.W2, t0, lane);
        float sx[KF];
        gather_read<KF>(a.xg, D, T, sx);
        const float eps_pg = sac_noise(a.b, a.b.noise_pg, STREAM_SAC_PG, trow, T.p);
        if (!accum) {   // the small tensors (first group only)
            small_copy_actor<NW * 64>(lds + F.small[0], a.act, PA.W1, PA, SA, tid);
            small_copy_critic<NW * 64>(lds + F.small[1], a.cri, PC.W1, PC, SC, tid);
        }
        TD3_BARRIER();   // the previous group is done with the LDS images; the small tensors are in
        if (wave == 0) xin_put<KF, XW>(xin, T, sx);   // the actor's input rows, for its first-layer weight gradient
        f32x4_t a1[PER], z2[PER], z3[PER], c1[PER], c2[PER];

        // ------------------------------------------------------------------ a_pg, lp = act.get_action_logprob(s): h1 in B0, h2 in B1
        float avg, raw;
        sac_actor_fwd<NT, PER, NW, KF, true>(a.act, PA, ac, SA, D, B0, B1, red, 0, wave, t0, lane, sx, wA, wB, a.cri + PC.W2, in, a1, z2, z3, avg, raw);
        const SacSample s = sac_sample(avg, raw, eps_pg);
        // ------------------------------------------------------------------ q1, q2 = cri_target.get_q1_q2(s, a_pg)
        float xt[KF];
        critic_input<KF>(sx, s.a, D, q, xt);
        target_critic_fwd<NT, PER, KF, S>(ct + SC.W1, ct, SC, a.cri + PC.W2, Dc, B2, t0, lane, xt, wA, wB, in, c1, c2);
        red_put(red, 2, wave, lane, head_partial<PER>(ct + SC.q1w, t0, lane, c2));
        red_put(red, 3, wave, lane, head_partial<PER>(ct + SC.q2w, t0, lane, c2));
        wload_t(wA, a.act + PA.W3, t0, lane);   // dA2 = W3^T dZ3
        TD3_BARRIER();
        // ------------------------------------------------------------------ backward through the critic to the action, from each sample's own head
        const float g = T.valid ? -invB : 0.f;   // d obj / d (min q + lp alpha)
        {
            const float q1 = red_get<NW>(red, 2, lane) + ct[SC.q1b], q2 = red_get<NW>(red, 3, lane) + ct[SC.q2b];
            const bool first = q1 <= q2;
            if (T.valid && wave == 0 && q == 0) q_acc += (first ? q1 : q2) + s.lp * alpha;
#pragma unroll
            for (int n = 0; n < PER; ++n) {
                const f32x4_t w1 = ld4(ct + SC.q1w + 16 * (t0 + n) + 4 * q), w2 = ld4(ct + SC.q2w + 16 * (t0 + n) + 4 * q);
                chain_put(B3, lane, t0 + n, gate4((first ? w1 : w2) * g, c2[n]));
            }
        }
        TD3_BARRIER();
        const float g_lp = g * alpha;                                              // d obj / d lp
        const float g_a = critic_to_action<NT, PER, NW, S>(ct + SC.W1, D, B3, red, 4, wave, t0, lane, wB, in, c1)
                          + g_lp * (-2.0f * s.a / s.corr);                         // + the tanh correction log(1.000001 - a^2)
        const float g_u = g_a * (1.0f - s.a * s.a);                                // tanh'; d u / d avg = 1
        const float g_raw = s.open ? g_u * s.std * s.eps + g_lp : 0.f;             // u = avg + exp(ls) eps, lp = ls + ...; the clamp's gate
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
        actor_body_bwd<GateHardswish, NT, PER, XW, S>(a.act + PA.W2, B0, B1, B2, B3, xin, t0, T, wA, wB, in, a1, z2, sl, SL);
    }
    tile_scalars_put(sl + SL.scalar_off, wave, tid, {q_acc});
}

// ======================================================================================================== host side
bool sac_supported(int D, int A, int md) { return A == 1 && D >= 1 && D <= kSacMaxD && (md == 64 || md == 128); }
int64_t sac_workspace_floats(int D, int md, int B) { return td3_workspace_floats(sac_actor_slab(D, md), D, md, B); }

struct SacKernels {   // td3_device.hpp: grad_dispatch
    using Args = SacGradArgs;
    template <int MD, int KF> static constexpr bool serves() { return MD <= 128 && KF == 2; }   // sac_supported, in the dispatch's terms
    static int lds_floats(int NT, int D) { return sac_lds(NT, D).total; }
    template <int MD, int DD, int NW, int KF> static constexpr auto critic() { return sac_critic_kernel<MD, DD, NW>; }
    template <int MD, int DD, int NW, int KF> static constexpr auto actor() { return sac_actor_kernel<MD, DD, NW>; }
};
int launch_sac_grad(bool critic, int md, const SacGradArgs& a, int grid, hipStream_t s) {
    if (!sac_supported(a.D, 1, md)) {
        set_error("no fused SAC instantiation for state_dim %d width %d", a.D, md);
        return PIME_ERR_ARG;
    }
    return grad_dispatch<SacKernels>(critic, md, a, grid, s);
}

}  // namespace pime
