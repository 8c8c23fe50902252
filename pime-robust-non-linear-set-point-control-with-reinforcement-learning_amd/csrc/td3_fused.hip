// One TD3 optimizer step as FOUR launches: critic gradients, critic apply, actor gradients, actor apply.
//
// replaces (reference, elegantrl/agent.py): AgentTD3.update_net's loop body (:314-331) -- get_obj_critic_raw
// (:361-370: minibatch gather, target actor + clamped smoothing noise (net.py:107-110), twin target heads + min, online twin
// forward, SmoothL1 x 2), obj_critic.backward(), cri_optimizer.step(), the delayed soft update of cri_target (:116-124),
// obj_actor = -cri_target(state, act(state)).mean() (:323-324; the reference differentiates through the TARGET critic's first head),
// obj_actor.backward(), act_optimizer.step(), the delayed soft update of act_target -- ~150 PyTorch / rocBLAS launches per
// optimizer step in round 3 (0.76 ms, 0.016 of the f32 matrix peak at batch 4 096).
//
// Shape of the problem: batch 4 096, nets of width 128 -- 0.48 MFLOP per sample, 2 GFLOP per step.  A sample tile per wave for the
// whole net (the PPO kernels' decomposition) would occupy 128 of 1 024 SIMDs.  Here a WORKGROUP owns one 16-sample tile and its
// NW waves (8 at width 128: two per SIMD; 4 at width 64) split every layer's OUTPUT features (v_mfma_f32_16x16x4_f32; wave w computes
// output tiles [PER w, PER w + PER) of md / 16, PER = md / 16 / NW): batch 4 096 = 256 workgroups = every SIMD of the chip busy.  Consequences:
//   * a weight element is used by exactly ONE wave of a workgroup, once: weights go global -> registers (16-byte row pieces of the
//     nn.Linear tensors themselves: a lane's four consecutive k values of an output row are one global_load_dwordx4), a layer ahead
//     of their use.  No packed images, no LDS staging, nothing to re-pack after an optimizer step.
//   * the layer's activation meets in LDS ("chain layout": tile t, lane group q, sample j, 4 registers = features 16 t + 4 q + r;
//     lane groups 72 floats apart): written as the accumulators stand (one ds_write_b128 per tile), read back by every wave as the
//     next layer's B operands (one ds_read_b128 per tile), and read again -- the same image, conflict-free ds_read_b32 -- as BOTH
//     operands of the weight gradients dW = dZ^T H, which contract over the tile's 16 samples (4 k-steps per 16 x 16 block).
//   * dX = W^T dZ reads W by columns (four dword loads where the forward has one 16-byte load).
//   * every workgroup leaves one partial gradient (slab, block-major in accumulator order); td3_apply_kernel sums the slabs in slab
//     order (bit-reproducible), applies torch.optim.Adam to the element it has just reduced and, on delayed steps, the soft target
//     update -- the parameters are the only copy of the weights, so that is all an optimizer step has to write.
// The minibatch rows come from an index table [steps][B]; the row of a step is a launch argument (a captured graph of an update's
// steps bakes each row into its nodes: no launch advances shared state); the smoothing noise comes from a table of normals (parity
// tests inject the reference's draws) or from Philox stream 3 in the kernel.
// Wider shapes: the Stacking observations (D up to 31) take the first layers in eight k-steps instead of two
// (template KF); width 256 keeps the decomposition -- eight waves, two output tiles each -- but streams the md x md weights in k-slices
// (Wts / wlayer: a register block of a layer would be 128 VGPRs), forms the md x md weight gradients in column slices, and at KF = 8
// reads the first-layer weights from global memory (they do not fit beside the chain images in LDS).  The round-4 instantiations
// (width 64 / 128, D <= 7) compile to the same arithmetic as before.
//
// What is this file's own: the two kernels' sequence -- which net runs where, the sv[] staging of the small tensors behind the index
// loads (round-4 shapes), the ReLU actor's forward, the smoothed target action and the label, the seed of the actor objective's
// backward (the target critic's first head) and the actor's single head -- and td3_apply_kernel, which SAC uses too.  Everything a
// SAC step (sac_fused.hip) does the same way is in td3_device.hpp: the tile context, the gather, the twin target heads, the online
// twin-critic step, the target critic's forward and its backward to the action, the actor body's backward, the launch dispatch.
#include "td3_device.hpp"

namespace pime {

// ======================================================================================================== critic gradients
// DD: the state width as a compile-time constant (3: pH, 4: water tank Integrator), 0: read from the arguments.  With DD fixed every
// offset of the parameter / slab / LDS layouts folds into an immediate; as run-time values they are ~100 live scalars that hipcc
// spills through VGPR lanes (v_readlane / v_writelane) and re-derives with scalar arithmetic in every phase.
template <int MD, int DD, int NW, int KF>
__global__ __launch_bounds__(NW * 64, 1) void td3_critic_kernel(Td3GradArgs a) {
    constexpr int NT = MD / 16, PER = NT / NW;
    static_assert(PER >= 1 && PER * NW == NT, "the waves split a layer's output tiles evenly");
    static_assert(DD == 0 || td3_first_ksteps(DD) == KF, "first-layer k-steps of the compiled-in state width");
    constexpr bool S = MD == 256;                     // streamed md x md weights (Wts)
    constexpr bool W1G = MD == 256 && KF == 8;        // first-layer weights read from global memory (td3_w1_global)
    constexpr bool GEN = KF == 8 || MD == 256;        // small tensors staged by small_copy (the round-4 shapes: sv[] below)
    constexpr int XW = KF == 2 ? 16 : 32;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int D = DD ? DD : a.D, Dc = D + 1;
    const Td3Lds F = td3_lds(NT, D);
    float* const B0 = lds + F.buf[0];
    float* const B1 = lds + F.buf[1];
    float* const B2 = lds + F.buf[2];
    float* const xin = lds + F.xin;
    float* const red = lds + F.red;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t0 = wave * PER;
    const Td3ActorOff PA = td3_actor_off(D, MD);
    const Td3CriticOff PC = td3_critic_off(D, MD);
    const Td3SmallActor SA = td3_small_actor(D, MD);
    const Td3SmallCritic SC = td3_small_critic(D, MD);
    const float* const at = lds + F.small[0];   // target actor, small tensors
    const float* const cr = lds + F.small[1];   // online critic
    const float* const ct = lds + F.small[2];   // target critic
    const Td3SlabLayout SL = td3_critic_slab(D, MD);
    const float invB = 1.0f / (float)a.b.B;
    const long long trow = a.b.row;
    float* const sl = a.slab + (size_t)blockIdx.x * a.stride;
    float loss_acc = 0.f;   // wave 0, lanes 0..15: this workgroup's loss terms

#pragma unroll 1
    for (int group = blockIdx.x; group < a.ngroups; group += gridDim.x) {
        const Td3Tile T = td3_tile(tid, group, a.b.B);
        const int lane = T.lane;
        Td3Gather<KF> G;
        gather_index(G, a.b, T);
        Wts<NT, PER, S> wA, wB;
        f32x4_t in[NT];
        wload(wA, a.act + PA.W2, t0, lane);   // the first md x md weights: in flight behind the gather's two round trips
        // the nets' small tensors ride behind the index loads (first group only): seven 16-byte loads per thread, one round trip
        const bool stage = !T.accum;
        const int nA0 = (PA.W2 - PA.W1) / 4, nA1 = MD / 4, nA2 = (PA.total - PA.b3) / 4, nC0 = (PC.W2 - PC.W1) / 4, nC1 = (PC.total - PC.b2) / 4;
        f32x4_t sv[9];
        if (!GEN && stage) {
            sv[0] = small_load(a.act + PA.W1, nA0, tid); sv[1] = small_load(a.act + PA.b2, nA1, tid); sv[2] = small_load(a.act + PA.b3, nA2, tid);
            sv[3] = small_load(a.cri + PC.W1, nC0, tid); sv[4] = small_load(a.cri + PC.b2, nC1, tid);
            sv[5] = small_load(a.cri_target + PC.W1, nC0, tid); sv[6] = small_load(a.cri_target + PC.b2, nC1, tid);
            sv[7] = small_load(a.cri + PC.W1 + 1024, nC0 - 256, tid); sv[8] = small_load(a.cri_target + PC.W1 + 1024, nC0 - 256, tid);   // D = 7 only
        }
        gather_rows(G, a.b, D, T);
        const float eps = td3_noise(a.b, trow, T.p);
        if (!GEN && stage) {
            float* const w = lds + F.small[0];
            small_store(w + SA.W1, nA0, tid, sv[0]); small_store(w + SA.b2, nA1, tid, sv[1]); small_store(w + SA.b3, nA2, tid, sv[2]);
            float* const c = lds + F.small[1];
            small_store(c + SC.W1, nC0, tid, sv[3]); small_store(c + SC.b2, nC1, tid, sv[4]);
            float* const t = lds + F.small[2];
            small_store(t + SC.W1, nC0, tid, sv[5]); small_store(t + SC.b2, nC1, tid, sv[6]);
            small_store(c + SC.W1 + 1024, nC0 - 256, tid, sv[7]); small_store(t + SC.W1 + 1024, nC0 - 256, tid, sv[8]);
        }
        if (GEN && stage) {
            const int a0 = W1G ? PA.b1 : PA.W1, c0 = W1G ? PC.b1 : PC.W1;
            small_copy_actor<NW * 64>(lds + F.small[0], a.act, a0, PA, SA, tid);
            small_copy_critic<NW * 64>(lds + F.small[1], a.cri, c0, PC, SC, tid);
            small_copy_critic<NW * 64>(lds + F.small[2], a.cri_target, c0, PC, SC, tid);
        }
        TD3_BARRIER();   // the previous group is done with the LDS images; the small tensors are in
        gather_publish<KF, XW>(G, D, T, wave, xin, a.xg);

        // ------------------------------------------------------------------ next_a = clamp(tanh(act_target(s')) + clamp(noise))
        {
            f32x4_t h[PER];
            layer_first<PER, KF>(W1G ? a.act + PA.W1 : at + SA.W1, at + SA.b1, D, t0, lane, G.nx, h);
#pragma unroll
            for (int n = 0; n < PER; ++n) chain_put(B0, lane, t0 + n, relu4(h[n]));
        }
        wload(wB, a.act + PA.W3, t0, lane);
        f32x4_t hb[PER];   // the next layer's accumulators, initialised with its bias in front of the barrier
        bias_get<PER>(at + SA.b2, t0, lane, hb);
        TD3_BARRIER();
        chain_get<NT>(B0, lane, in);
        {
            wlayer(wA, in, hb);
#pragma unroll
            for (int n = 0; n < PER; ++n) chain_put(B1, lane, t0 + n, relu4(hb[n]));
        }
        wload(wA, a.cri_target + PC.W2, t0, lane);
        bias_get<PER>(at + SA.b3, t0, lane, hb);
        TD3_BARRIER();
        chain_get<NT>(B1, lane, in);
        float next_a;
        {
            f32x4_t (&h)[PER] = hb;
            wlayer(wB, in, h);
#pragma unroll
            for (int n = 0; n < PER; ++n) h[n] = relu4(h[n]);
            red_put(red, 0, wave, lane, head_partial<PER>(at + SA.w4, t0, lane, h));
            TD3_BARRIER();
            const float pre = red_get<NW>(red, 0, lane) + at[SA.b4];
            const float nz = fminf(fmaxf(eps * a.b.policy_noise, -a.b.noise_clip), a.b.noise_clip);   // net.py:109
            next_a = fminf(fmaxf(tanhf(pre) + nz, -1.0f), 1.0f);
        }
        // ------------------------------------------------------------------ q_label = r + mask * min(cri_target twin heads)(s', next_a)
        wload(wB, a.cri + PC.W2, t0, lane);
        float xt[KF], tq1, tq2;
        critic_input<KF>(G.nx, next_a, D, T.q, xt);
        twin_heads<NT, PER, NW, KF, S>(W1G ? a.cri_target + PC.W1 : ct + SC.W1, ct, SC, Dc, B0, red, 1, wave, t0, lane, xt, wA, in, tq1, tq2);
        const float label = G.reward + G.mask * fminf(tq1, tq2);
        // ------------------------------------------------------------------ online twin critic on (s, a): loss, backward, weight gradients
        online_critic_step<NT, PER, NW, KF, XW, S>(W1G ? a.cri + PC.W1 : cr + SC.W1, cr, SC, a.cri + PC.W2, Dc, B0, B1, B2, xin, red, 3, wave, t0,
                                                   T, G.xs, label, invB, wA, wB, in, sl, SL, loss_acc);
    }
    tile_scalars_put(sl + SL.scalar_off, wave, tid, {loss_acc});
}

// ======================================================================================================== actor gradients
// obj_actor = -mean(cri_target.q1(s, tanh(act(s))))  (agent.py:323-324), differentiated down to the actor's parameters
template <int MD, int DD, int NW, int KF>
__global__ __launch_bounds__(NW * 64, 1) void td3_actor_kernel(Td3GradArgs a) {
    constexpr int NT = MD / 16, PER = NT / NW;
    static_assert(PER >= 1 && PER * NW == NT, "the waves split a layer's output tiles evenly");
    static_assert(DD == 0 || td3_first_ksteps(DD) == KF, "first-layer k-steps of the compiled-in state width");
    constexpr bool S = MD == 256;                     // streamed md x md weights (Wts)
    constexpr bool W1G = MD == 256 && KF == 8;        // first-layer weights read from global memory (td3_w1_global)
    constexpr bool GEN = KF == 8 || MD == 256;        // small tensors staged by small_copy (the round-4 shapes: sv[] below)
    constexpr int XW = KF == 2 ? 16 : 32;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int D = DD ? DD : a.D, Dc = D + 1;
    const Td3Lds F = td3_lds(NT, D);
    float* const B0 = lds + F.buf[0];
    float* const B1 = lds + F.buf[1];
    float* const B2 = lds + F.buf[2];
    float* const B3 = lds + F.buf[3];
    float* const xin = lds + F.xin;
    float* const red = lds + F.red;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t0 = wave * PER;
    const Td3ActorOff PA = td3_actor_off(D, MD);
    const Td3CriticOff PC = td3_critic_off(D, MD);
    const Td3SmallActor SA = td3_small_actor(D, MD);
    const Td3SmallCritic SC = td3_small_critic(D, MD);
    const float* const ac = lds + F.small[0];   // online actor, small tensors
    const float* const ct = lds + F.small[1];   // target critic
    const float* const ctW1 = W1G ? a.cri + PC.W1 : ct + SC.W1;   // its first layer
    const Td3SlabLayout SL = td3_actor_slab(D, MD);
    const float invB = 1.0f / (float)a.b.B;
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
        const bool stage = !accum;   // the small tensors ride along (first group only)
        const int nA0 = (PA.W2 - PA.W1) / 4, nA1 = MD / 4, nA2 = (PA.total - PA.b3) / 4, nC0 = (PC.W2 - PC.W1) / 4, nC1 = (PC.total - PC.b2) / 4;
        f32x4_t sv[6];
        if (!GEN && stage) {
            sv[0] = small_load(a.act + PA.W1, nA0, tid); sv[1] = small_load(a.act + PA.b2, nA1, tid); sv[2] = small_load(a.act + PA.b3, nA2, tid);
            sv[3] = small_load(a.cri + PC.W1, nC0, tid); sv[4] = small_load(a.cri + PC.b2, nC1, tid);
            sv[5] = small_load(a.cri + PC.W1 + 1024, nC0 - 256, tid);   // D = 7 only
        }
        if (!GEN && stage) {
            float* const w = lds + F.small[0];
            small_store(w + SA.W1, nA0, tid, sv[0]); small_store(w + SA.b2, nA1, tid, sv[1]); small_store(w + SA.b3, nA2, tid, sv[2]);
            float* const c = lds + F.small[1];
            small_store(c + SC.W1, nC0, tid, sv[3]); small_store(c + SC.b2, nC1, tid, sv[4]);
            small_store(c + SC.W1 + 1024, nC0 - 256, tid, sv[5]);
        }
        if (GEN && stage) {
            small_copy_actor<NW * 64>(lds + F.small[0], a.act, W1G ? PA.b1 : PA.W1, PA, SA, tid);
            small_copy_critic<NW * 64>(lds + F.small[1], a.cri, W1G ? PC.b1 : PC.W1, PC, SC, tid);
        }
        TD3_BARRIER();   // the previous group is done with the LDS images; the small tensors are in
        if (wave == 0) xin_put<KF, XW>(xin, T, sx);   // the actor's input rows, for its first-layer weight gradient
        f32x4_t a1[PER], a2[PER], a3[PER], c1[PER], c2[PER];

        // ------------------------------------------------------------------ action = tanh(act(s))
        layer_first<PER, KF>(W1G ? a.act + PA.W1 : ac + SA.W1, ac + SA.b1, D, t0, lane, sx, a1);
#pragma unroll
        for (int n = 0; n < PER; ++n) { a1[n] = relu4(a1[n]); chain_put(B0, lane, t0 + n, a1[n]); }
        wload(wB, a.act + PA.W3, t0, lane);
        bias_get<PER>(ac + SA.b2, t0, lane, a2);   // a layer's accumulators start as its bias, read in front of the barrier
        TD3_BARRIER();
        chain_get<NT>(B0, lane, in);
        wlayer(wA, in, a2);
#pragma unroll
        for (int n = 0; n < PER; ++n) { a2[n] = relu4(a2[n]); chain_put(B1, lane, t0 + n, a2[n]); }
        wload(wA, a.cri + PC.W2, t0, lane);
        bias_get<PER>(ac + SA.b3, t0, lane, a3);
        TD3_BARRIER();
        chain_get<NT>(B1, lane, in);
        wlayer(wB, in, a3);
#pragma unroll
        for (int n = 0; n < PER; ++n) a3[n] = relu4(a3[n]);
        red_put(red, 0, wave, lane, head_partial<PER>(ac + SA.w4, t0, lane, a3));
        TD3_BARRIER();
        const float act = tanhf(red_get<NW>(red, 0, lane) + ac[SA.b4]);
        // ------------------------------------------------------------------ q1 = cri_target.q1(s, action)
        float xt[KF];
        critic_input<KF>(sx, act, D, q, xt);
        target_critic_fwd<NT, PER, KF, S>(ctW1, ct, SC, a.cri + PC.W2, Dc, B2, t0, lane, xt, wA, wB, in, c1, c2);
        red_put(red, 1, wave, lane, head_partial<PER>(ct + SC.q1w, t0, lane, c2));   // (the value itself only feeds the logged objective)
        // ------------------------------------------------------------------ backward through the critic to the action, from the first head
        const float g = T.valid ? -invB : 0.f;   // d(-mean q1) / d q1
#pragma unroll
        for (int n = 0; n < PER; ++n) {
            const f32x4_t wq = ld4(ct + SC.q1w + 16 * (t0 + n) + 4 * q);
            chain_put(B3, lane, t0 + n, gate4(wq * g, c2[n]));
        }
        wload_t(wA, a.act + PA.W3, t0, lane);   // dA2 = W3^T dZ3
        TD3_BARRIER();
        if (T.valid && wave == 0 && q == 0) q_acc += red_get<NW>(red, 1, lane) + ct[SC.q1b];
        const float dpre = critic_to_action<NT, PER, NW, S>(ctW1, D, B3, red, 2, wave, t0, lane, wB, in, c1) * (1.0f - act * act);   // tanh'
        // ------------------------------------------------------------------ actor backward + weight gradients
        {
            f32x4_t v[PER], dz[PER];
#pragma unroll
            for (int n = 0; n < PER; ++n) {
                const f32x4_t w4 = ld4(ac + SA.w4 + 16 * (t0 + n) + 4 * q);
                v[n] = a3[n] * dpre;
                dz[n] = gate4(w4 * dpre, a3[n]);
                chain_put(B2, lane, t0 + n, dz[n]);
            }
            vec_grad<PER>(sl + SL.seg[6].slab_off, t0, lane, v, accum);    // net.6 weight
            vec_grad<PER>(sl + SL.seg[5].slab_off, t0, lane, dz, accum);   // net.4 bias
            if (wave == 0) {
                const float bg = row_sum16(dpre);
                if (lane == 0) {
                    float* pb = sl + SL.seg[7].slab_off;
                    pb[0] = accum ? pb[0] + bg : bg;
                }
            }
        }
        actor_body_bwd<GateRelu, NT, PER, XW, S>(a.act + PA.W2, B0, B1, B2, B3, xin, t0, T, wA, wB, in, a1, a2, sl, SL);
    }
    tile_scalars_put(sl + SL.scalar_off, wave, tid, {q_acc});
}

// ======================================================================================================== slab reduction + Adam + soft update
// Workgroup = kApplyWords (64) consecutive 16-byte words of the slab layout x kApplyGroups (8) slab groups (the first version: 16 x 16;
// 1 KB contiguous per slab and 32 loads per thread in flight read the freshly written slabs 23 % faster, see the sweep below):
// thread (g, l) sums word l of slabs g, g + 8, ... with
// ALL of them in flight at once (the slabs were written by other compute units a kernel ago: every load is an Infinity-Cache / HBM
// round trip, and the launch is a few hundred workgroups of one such round trip each -- the first version, 64 words x 4 groups with
// four loads in flight, took 11.5 us of a 78 us optimizer step); the 16 partial sums meet in LDS and are combined in group order
// (bit-reproducible); the threads of group 0 then own four gradient elements each: they write them, apply torch.optim.Adam (defaults:
// no weight decay, no amsgrad) to their parameters and, on a delayed step, target = tau * param + (1 - tau) * target (agent.py:116-124,
// the reference's operand order).
// Words x threads swept at the end of round 4 (us per launch): 16x256 9.6, 8x256 11.6, 32x256 8.7, 64x256 8.2, 128x256 10.6,
// 32x512 8.6, 64x512 7.4, 128x512 9.1, 256x512 14.8, 64x1024 7.5, 32x1024 12.8 (profiles/r04_w_td3_apply_shape_sweep.txt)
constexpr int kApplyThreads = 512;
constexpr int kApplyWords = 64, kApplyGroups = kApplyThreads / kApplyWords;
constexpr int kApplyBatch = 256 / kApplyGroups > 32 ? 32 : 256 / kApplyGroups;   // slab loads a thread keeps in flight: one batch covers 256 slabs
// SAC: the temperature's Adam step rides on the scalar word's finisher (sac_fused.hip; Td3ApplyArgs::temp) -- compiled out for TD3.
template <bool SAC>
__global__ __launch_bounds__(kApplyThreads) void td3_apply_kernel(Td3ApplyArgs a) {
    __shared__ float4 part[kApplyGroups][kApplyWords];
    __shared__ float adam_sh[3];   // [1] step size, [2] sqrt of the second bias correction
    const int tid = threadIdx.x, l = tid & (kApplyWords - 1), g = tid / kApplyWords;
    const int nwords = a.L.stride / 4;
    const int unit = blockIdx.x * kApplyWords + l;
    const bool finisher = g == 0 && unit < nwords;
    if (tid == 64) {   // Adam's bias corrections, off the finishers' critical path.  The step number is a launch argument + a base the
        // host moves once per update: no workgroup writes shared state, so the launch needs no arrival counter (the first version's
        // atomic on one word cost ~12 ns per workgroup: 2.5 us of its 11.5 with 200 workgroups, 10 us with 850)
        const double t = (double)a.step[0] + (double)a.row + 1.0;
        adam_sh[1] = a.lr / (float)(1.0 - pow((double)a.b1, t));
        adam_sh[2] = (float)sqrt(1.0 - pow((double)a.b2, t));
    }
    const bool soft = a.soft != 0;
    // which elements a finisher owns
    long long flat[4] = {-1, -1, -1, -1};
    bool scalar_word = false;
    if (finisher) {
        const int off = unit * 4;
        if (off >= a.L.scalar_off) scalar_word = true;
        else {
            int si = 0;
            while (si + 1 < a.L.nseg && off >= a.L.seg[si + 1].slab_off) ++si;
            const Td3Seg sg = a.L.seg[si];
            const int u = (off - sg.slab_off) / 4;
            if (u < sg.n4) {
                if (sg.tb > 0) {
                    const int blk = u >> 6, ln = u & 63;
                    const int row = (blk / sg.tb) * 16 + 4 * (ln >> 4), col = (blk % sg.tb) * 16 + (ln & 15);
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (col < sg.ncols) flat[k] = sg.flat_off + (long long)(row + k) * sg.ldw + col;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (u * 4 + k < sg.n) flat[k] = sg.flat_off + u * 4 + k;
                }
            }
        }
    }
    // optimizer state of those elements, requested before the slab loads
    float pm[4] = {0.f, 0.f, 0.f, 0.f}, pv[4] = {0.f, 0.f, 0.f, 0.f}, pp[4] = {0.f, 0.f, 0.f, 0.f}, pt[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (flat[k] >= 0) {
            pm[k] = a.exp_avg[flat[k]]; pv[k] = a.exp_avg_sq[flat[k]]; pp[k] = a.param[flat[k]];
            if (soft) pt[k] = a.target[flat[k]];
        }
    float gin[4] = {0.f, 0.f, 0.f, 0.f};   // mode 2: the (all-reduced) gradient stands in for the slab sums
    if (a.mode == 2) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (flat[k] >= 0) gin[k] = a.grad[flat[k]];
    }
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (unit < nwords && a.mode != 2) {
        const float* base = a.slab + (size_t)unit * 4;
        const size_t stride = (size_t)a.L.stride;
        int s = g;
        for (; s + (kApplyBatch - 1) * kApplyGroups < a.nslabs; s += kApplyBatch * kApplyGroups) {   // kApplyBatch loads in flight (256 slabs: one batch)
            float4 v[kApplyBatch];
#pragma unroll
            for (int k = 0; k < kApplyBatch; ++k) v[k] = *reinterpret_cast<const float4*>(base + (size_t)(s + kApplyGroups * k) * stride);
#pragma unroll
            for (int k = 0; k < kApplyBatch; ++k) { acc.x += v[k].x; acc.y += v[k].y; acc.z += v[k].z; acc.w += v[k].w; }
        }
        for (; s + 3 * kApplyGroups < a.nslabs; s += 4 * kApplyGroups) {
            float4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = *reinterpret_cast<const float4*>(base + (size_t)(s + kApplyGroups * k) * stride);
#pragma unroll
            for (int k = 0; k < 4; ++k) { acc.x += v[k].x; acc.y += v[k].y; acc.z += v[k].z; acc.w += v[k].w; }
        }
        for (; s < a.nslabs; s += kApplyGroups) {
            const float4 v = *reinterpret_cast<const float4*>(base + (size_t)s * stride);
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
    }
    part[g][l] = acc;
    __syncthreads();
    const float step_size = adam_sh[1], bc2_sqrt = adam_sh[2];
    if (finisher) {
        float4 t = part[0][l];
        for (int w = 1; w < kApplyGroups; ++w) { const float4 v = part[w][l]; t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w; }
        const float gv[4] = {a.mode == 2 ? gin[0] : t.x, a.mode == 2 ? gin[1] : t.y, a.mode == 2 ? gin[2] : t.z, a.mode == 2 ? gin[3] : t.w};
        if (scalar_word) {
            if (a.loss && a.mode != 2) {
                const float val = (a.loss_slot == 0 ? -gv[0] : gv[0]) * a.inv_B;
                a.loss[a.loss_slot] += val;
                a.loss[a.loss_last + a.loss_slot] = val;
            }
            if (SAC && a.temp.alpha_log && a.mode != 2) {   // the temperature's objective, gradient and Adam step (td3.hpp)
                const double t = (double)a.step[0] + (double)a.row + 1.0;
                const float ss = a.temp.lr / (float)(1.0 - pow((double)a.temp.b1, t)), bs = (float)sqrt(1.0 - pow((double)a.temp.b2, t));
                const float al = a.temp.alpha_log[0], g = gv[1] * a.inv_B - a.temp.target_entropy;
                const float mi = a.temp.exp_avg[0] + (g - a.temp.exp_avg[0]) * (1.0f - a.temp.b1);
                const float vi = a.temp.exp_avg_sq[0] * a.temp.b2 + g * g * (1.0f - a.temp.b2);
                const float an = al - ss * (mi / (sqrtf(vi) / bs + a.temp.eps));
                a.temp.exp_avg[0] = mi;
                a.temp.exp_avg_sq[0] = vi;
                a.temp.alpha_log[0] = an;
                if (a.loss) {
                    const float oa = al * g, alpha = expf(an);
                    a.loss[2] += oa; a.loss[a.loss_last + 2] = oa;
                    a.loss[3] += alpha; a.loss[a.loss_last + 3] = alpha;
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (flat[k] < 0) continue;
                const long long e = flat[k];
                if (a.mode != 2) a.grad[e] = gv[k];
                if (a.mode == 1) continue;
                const float mi = pm[k] + (gv[k] - pm[k]) * (1.0f - a.b1);
                const float vi = pv[k] * a.b2 + gv[k] * gv[k] * (1.0f - a.b2);
                a.exp_avg[e] = mi;
                a.exp_avg_sq[e] = vi;
                const float pn = pp[k] - step_size * (mi / (sqrtf(vi) / bc2_sqrt + a.eps));
                a.param[e] = pn;
                if (soft) a.target[e] = pn * a.tau + pt[k] * (1.0f - a.tau);
            }
        }
    }
}

// ======================================================================================================== host side
int td3_grid(int B) {   // one 16-sample group per workgroup, at most kTd3MaxSlabs
    const int ngroups = (B + kTd3Tile - 1) / kTd3Tile;
    return ngroups < kTd3MaxSlabs ? ngroups : kTd3MaxSlabs;
}
int64_t td3_workspace_floats(const Td3SlabLayout& actor, int D, int md, int B) {
    const int64_t g = td3_grid(B);
    // slabs + the gathered rows [B][td3_xg_stride(D)]
    return g * (actor.stride + td3_critic_slab(D, md).stride) + (int64_t)B * td3_xg_stride(D);
}
int64_t td3_workspace_floats(int D, int md, int B) { return td3_workspace_floats(td3_actor_slab(D, md), D, md, B); }
bool td3_supported(int D, int A, int md) { return A == 1 && D >= 1 && D <= kTd3MaxD && (md == 64 || md == 128 || md == 256); }

struct Td3Kernels {   // td3_device.hpp: grad_dispatch
    using Args = Td3GradArgs;
    template <int MD, int KF> static constexpr bool serves() { return true; }
    static int lds_floats(int NT, int D) { return td3_lds(NT, D).total; }
    template <int MD, int DD, int NW, int KF> static constexpr auto critic() { return td3_critic_kernel<MD, DD, NW, KF>; }
    template <int MD, int DD, int NW, int KF> static constexpr auto actor() { return td3_actor_kernel<MD, DD, NW, KF>; }
};
int launch_td3_grad(bool critic, int md, const Td3GradArgs& a, int grid, hipStream_t s) {
    if (md != 64 && md != 128 && md != 256) {
        set_error("no fused TD3 instantiation for width %d", md);
        return PIME_ERR_ARG;
    }
    return grad_dispatch<Td3Kernels>(critic, md, a, grid, s);
}
int launch_td3_apply(const Td3ApplyArgs& a, hipStream_t s) {
    const int nwords = a.L.stride / 4;
    if (a.temp.alpha_log) hipLaunchKernelGGL(td3_apply_kernel<true>, dim3((nwords + kApplyWords - 1) / kApplyWords), dim3(kApplyThreads), 0, s, a);
    else hipLaunchKernelGGL(td3_apply_kernel<false>, dim3((nwords + kApplyWords - 1) / kApplyWords), dim3(kApplyThreads), 0, s, a);
    PIME_HIP_TRY(hipGetLastError());
    return PIME_OK;
}

}  // namespace pime
