// One TD3 optimizer step as FOUR launches: critic gradients, critic apply, actor gradients, actor apply.
//
// replaces (reference, /root/reference/elegantrl/agent.py): AgentTD3.update_net's loop body (:314-331) -- get_obj_critic_raw
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
    constexpr int XW = KF == 2 ? 16 : 32, CT = XW / 16, XG = 4 * KF;
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
        int lane = tid & 63;
        asm volatile("" : "+v"(lane));
        const int j = lane & 15, q = lane >> 4;
        const bool accum = group != (int)blockIdx.x;
        const int pos = group * kTd3Tile + j;
        const bool valid = pos < a.b.B;
        const int p = valid ? pos : a.b.B - 1;
        const long long row = a.b.idx[(size_t)trow * a.b.B + p], nrow = a.b.nxt[(size_t)trow * a.b.B + p];
        Wts<NT, PER, S> wA, wB;
        f32x4_t in[NT];
        wload(wA, a.act + PA.W2, t0, lane);   // the first md x md weights: in flight behind the gather's two round trips
        // the nets' small tensors ride behind the index loads (first group only): seven 16-byte loads per thread, one round trip
        const bool stage = !accum;
        const int nA0 = (PA.W2 - PA.W1) / 4, nA1 = MD / 4, nA2 = (PA.total - PA.b3) / 4, nC0 = (PC.W2 - PC.W1) / 4, nC1 = (PC.total - PC.b2) / 4;
        f32x4_t sv[9];
        if (!GEN && stage) {
            sv[0] = small_load(a.act + PA.W1, nA0, tid); sv[1] = small_load(a.act + PA.b2, nA1, tid); sv[2] = small_load(a.act + PA.b3, nA2, tid);
            sv[3] = small_load(a.cri + PC.W1, nC0, tid); sv[4] = small_load(a.cri + PC.b2, nC1, tid);
            sv[5] = small_load(a.cri_target + PC.W1, nC0, tid); sv[6] = small_load(a.cri_target + PC.b2, nC1, tid);
            sv[7] = small_load(a.cri + PC.W1 + 1024, nC0 - 256, tid); sv[8] = small_load(a.cri_target + PC.W1 + 1024, nC0 - 256, tid);   // D = 7 only
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
        const float eps = td3_noise(a.b, trow, p);
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
            small_copy<NW * 64>(lds + F.small[0], a.act, a0, PA.W2, tid);
            small_copy<NW * 64>(lds + F.small[0] + SA.b2, a.act, PA.b2, PA.W3, tid);
            small_copy<NW * 64>(lds + F.small[0] + SA.b3, a.act, PA.b3, PA.total, tid);
            small_copy<NW * 64>(lds + F.small[1], a.cri, c0, PC.W2, tid);
            small_copy<NW * 64>(lds + F.small[1] + SC.b2, a.cri, PC.b2, PC.total, tid);
            small_copy<NW * 64>(lds + F.small[2], a.cri_target, c0, PC.W2, tid);
            small_copy<NW * 64>(lds + F.small[2] + SC.b2, a.cri_target, PC.b2, PC.total, tid);
        }
        TD3_BARRIER();   // the previous group is done with the LDS images; the small tensors are in
        // the online critic's input [s, a, 0 ..]: column q / 4 + q of sample j (this lane's first-layer B operands)
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

        // ------------------------------------------------------------------ next_a = clamp(tanh(act_target(s')) + clamp(noise))
        {
            f32x4_t h[PER];
            layer_first<PER, KF>(W1G ? a.act + PA.W1 : at + SA.W1, at + SA.b1, D, t0, lane, nx, h);
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
        float label;
        {
            float xt[KF];
#pragma unroll
            for (int k = 0; k < KF; ++k) xt[k] = 4 * k + q < D ? nx[k] : (4 * k + q == D ? next_a : 0.f);
            f32x4_t h[PER];
            layer_first<PER, KF>(W1G ? a.cri_target + PC.W1 : ct + SC.W1, ct + SC.b1, Dc, t0, lane, xt, h);
#pragma unroll
            for (int n = 0; n < PER; ++n) chain_put(B0, lane, t0 + n, relu4(h[n]));
            bias_get<PER>(ct + SC.b2, t0, lane, h);
            TD3_BARRIER();
            chain_get<NT>(B0, lane, in);
            wlayer(wA, in, h);
#pragma unroll
            for (int n = 0; n < PER; ++n) h[n] = relu4(h[n]);
            red_put(red, 1, wave, lane, head_partial<PER>(ct + SC.q1w, t0, lane, h));
            red_put(red, 2, wave, lane, head_partial<PER>(ct + SC.q2w, t0, lane, h));
            TD3_BARRIER();
            const float tq1 = red_get<NW>(red, 1, lane) + ct[SC.q1b], tq2 = red_get<NW>(red, 2, lane) + ct[SC.q2b];
            label = reward + mask * fminf(tq1, tq2);
        }
        // ------------------------------------------------------------------ online twin critic on (s, a): forward
        f32x4_t h1[PER], h2[PER];
        {
            layer_first<PER, KF>(W1G ? a.cri + PC.W1 : cr + SC.W1, cr + SC.b1, Dc, t0, lane, xs, h1);
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
        red_put(red, 3, wave, lane, head_partial<PER>(cr + SC.q1w, t0, lane, h2));
        red_put(red, 4, wave, lane, head_partial<PER>(cr + SC.q2w, t0, lane, h2));
        TD3_BARRIER();
        // ------------------------------------------------------------------ SmoothL1 x 2 (beta = 1, mean) and its gradient
        float g1 = 0.f, g2 = 0.f;
        {
            const float d1 = red_get<NW>(red, 3, lane) + cr[SC.q1b] - label, d2 = red_get<NW>(red, 4, lane) + cr[SC.q2b] - label;
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
        dw_slab<NT, PER, S>(B2, B1, sl + SL.seg[2].slab_off, t0, lane, accum);   // net_sa.2 weight gradient
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
            f32x4_t acc[PER][CT];
            dw_first<PER, XW>(B0, xin, t0, lane, acc);
            float* seg = sl + SL.seg[0].slab_off;
#pragma unroll
            for (int n = 0; n < PER; ++n)
#pragma unroll
                for (int c = 0; c < CT; ++c) slab_put(seg + (((t0 + n) * CT + c) * 64 + lane) * 4, acc[n][c], accum);
        }
    }
    if (wave == 0) {
        const float t = row_sum16(loss_acc);
        if (tid == 0) st4(sl + SL.scalar_off, f32x4_t{t, 0.f, 0.f, 0.f});
    }
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
    constexpr int XW = KF == 2 ? 16 : 32, CT = XW / 16, XG = 4 * KF;
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
        int lane = tid & 63;
        asm volatile("" : "+v"(lane));
        const int j = lane & 15, q = lane >> 4;
        const bool accum = group != (int)blockIdx.x;
        const int pos = group * kTd3Tile + j;
        const bool valid = pos < a.b.B;
        const int p = valid ? pos : a.b.B - 1;
        Wts<NT, PER, S> wA, wB;
        f32x4_t in[NT];
        wload(wA, a.act + PA.W2, t0, lane);
        // the minibatch's state rows as the critic launch of this step gathered them (one round trip instead of index -> row)
        float sx[KF];
#pragma unroll
        for (int k = 0; k < KF; ++k) sx[k] = 4 * k + q < D ? a.xg[(size_t)p * XG + 4 * k + q] : 0.f;
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
            const int a0 = W1G ? PA.b1 : PA.W1, c0 = W1G ? PC.b1 : PC.W1;
            small_copy<NW * 64>(lds + F.small[0], a.act, a0, PA.W2, tid);
            small_copy<NW * 64>(lds + F.small[0] + SA.b2, a.act, PA.b2, PA.W3, tid);
            small_copy<NW * 64>(lds + F.small[0] + SA.b3, a.act, PA.b3, PA.total, tid);
            small_copy<NW * 64>(lds + F.small[1], a.cri, c0, PC.W2, tid);
            small_copy<NW * 64>(lds + F.small[1] + SC.b2, a.cri, PC.b2, PC.total, tid);
        }
        TD3_BARRIER();   // the previous group is done with the LDS images; the small tensors are in
        if (wave == 0) {   // the actor's input rows [16 samples][XW columns, zero beyond D] for its first-layer weight gradient
#pragma unroll
            for (int k = 0; k < XW / 4; ++k) xin[j * XW + 4 * k + q] = k < KF ? sx[k] : 0.f;
        }
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
        {
            float xt[KF];
#pragma unroll
            for (int k = 0; k < KF; ++k) xt[k] = 4 * k + q < D ? sx[k] : (4 * k + q == D ? act : 0.f);
            layer_first<PER, KF>(ctW1, ct + SC.b1, Dc, t0, lane, xt, c1);
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
        red_put(red, 1, wave, lane, head_partial<PER>(ct + SC.q1w, t0, lane, c2));   // (the value itself only feeds the logged objective)
        // ------------------------------------------------------------------ backward through the critic to the action
        const float g = valid ? -invB : 0.f;   // d(-mean q1) / d q1
#pragma unroll
        for (int n = 0; n < PER; ++n) {
            const f32x4_t wq = ld4(ct + SC.q1w + 16 * (t0 + n) + 4 * q);
            chain_put(B3, lane, t0 + n, gate4(wq * g, c2[n]));
        }
        wload_t(wA, a.act + PA.W3, t0, lane);   // dA2 = W3^T dZ3
        TD3_BARRIER();
        if (valid && wave == 0 && q == 0) q_acc += red_get<NW>(red, 1, lane) + ct[SC.q1b];
        chain_get<NT>(B3, lane, in);
        float dpre;
        {
            f32x4_t d[PER];
            zero4<PER>(d);
            wlayer(wB, in, d);
            float pa = 0.f;   // d obj / d action = sum_f W1[f][D] dZc1[f]
#pragma unroll
            for (int n = 0; n < PER; ++n) {
                d[n] = gate4(d[n], c1[n]);
#pragma unroll
                for (int r = 0; r < 4; ++r) pa = fmaf(d[n][r], ctW1[(16 * (t0 + n) + 4 * q + r) * Dc + D], pa);
            }
            pa += __shfl_xor(pa, 16);
            pa += __shfl_xor(pa, 32);
            red_put(red, 2, wave, lane, pa);
            TD3_BARRIER();
            dpre = red_get<NW>(red, 2, lane) * (1.0f - act * act);   // tanh'
        }
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
        wload_t(wB, a.act + PA.W2, t0, lane);   // dA1 = W2^T dZ2
        TD3_BARRIER();   // dZ3 published
        dw_slab<NT, PER, S>(B2, B1, sl + SL.seg[4].slab_off, t0, lane, accum);   // net.4: dZ3^T A2
        TD3_NO_HOIST();
        chain_get<NT>(B2, lane, in);
        {
            f32x4_t d[PER];
            zero4<PER>(d);
            wlayer(wA, in, d);
#pragma unroll
            for (int n = 0; n < PER; ++n) { d[n] = gate4(d[n], a2[n]); chain_put(B3, lane, t0 + n, d[n]); }
            vec_grad<PER>(sl + SL.seg[3].slab_off, t0, lane, d, accum);    // net.2 bias
        }
        TD3_BARRIER();   // dZ2 published
        dw_slab<NT, PER, S>(B3, B0, sl + SL.seg[2].slab_off, t0, lane, accum);   // net.2: dZ2^T A1
        TD3_NO_HOIST();
        chain_get<NT>(B3, lane, in);
        {
            f32x4_t d[PER];
            zero4<PER>(d);
            wlayer(wB, in, d);
#pragma unroll
            for (int n = 0; n < PER; ++n) { d[n] = gate4(d[n], a1[n]); chain_put(B1, lane, t0 + n, d[n]); }
            vec_grad<PER>(sl + SL.seg[1].slab_off, t0, lane, d, accum);    // net.0 bias
        }
        TD3_BARRIER();   // dZ1 published
        {
            f32x4_t acc[PER][CT];
            dw_first<PER, XW>(B1, xin, t0, lane, acc);
            float* seg = sl + SL.seg[0].slab_off;
#pragma unroll
            for (int n = 0; n < PER; ++n)
#pragma unroll
                for (int c = 0; c < CT; ++c) slab_put(seg + (((t0 + n) * CT + c) * 64 + lane) * 4, acc[n][c], accum);
        }
    }
    if (wave == 0) {
        const float t = row_sum16(q_acc);
        if (tid == 0) st4(sl + SL.scalar_off, f32x4_t{t, 0.f, 0.f, 0.f});
    }
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
int64_t td3_workspace_floats(int D, int md, int B) {
    const int64_t g = td3_grid(B);
    // slabs + the gathered rows [B][td3_xg_stride(D)]
    return g * (td3_actor_slab(D, md).stride + td3_critic_slab(D, md).stride) + (int64_t)B * td3_xg_stride(D);
}
bool td3_supported(int D, int A, int md) { return A == 1 && D >= 1 && D <= kTd3MaxD && (md == 64 || md == 128 || md == 256); }

// Waves per workgroup of the gradient kernels.  Width 64 has four output tiles: four waves, one per SIMD.  Widths 128 and 256: eight
// waves, two per SIMD, owning one / two of a layer's eight / sixteen output tiles (the non-MFMA instructions of one wave issue behind
// the other's MFMAs); at width 128 that measured 60.4 us per optimizer step against 63.1 on four waves (profiles/r04_u_td3_waves_ab.txt).
template <int MD, int DD, int KF>
static int launch_grad_d(bool critic, const Td3GradArgs& a, int grid, hipStream_t s) {
    constexpr int NW = MD == 64 ? 4 : 8;
    const size_t lds_bytes = sizeof(float) * (size_t)td3_lds(MD / 16, a.D).total;
    if (critic) hipLaunchKernelGGL((td3_critic_kernel<MD, DD, NW, KF>), dim3(grid), dim3(NW * 64), lds_bytes, s, a);
    else hipLaunchKernelGGL((td3_actor_kernel<MD, DD, NW, KF>), dim3(grid), dim3(NW * 64), lds_bytes, s, a);
    PIME_HIP_TRY(hipGetLastError());
    return PIME_OK;
}
template <int MD>
static int launch_grad(bool critic, const Td3GradArgs& a, int grid, hipStream_t s) {
    if (a.D == 3) return launch_grad_d<MD, 3, 2>(critic, a, grid, s);     // pH observation
    if (a.D == 4) return launch_grad_d<MD, 4, 2>(critic, a, grid, s);     // water-tank Integrator observation
    if (a.D == 12) return launch_grad_d<MD, 12, 8>(critic, a, grid, s);   // water-tank Stacking4
    if (a.D == 30) return launch_grad_d<MD, 30, 8>(critic, a, grid, s);   // water-tank Stacking10
    if (td3_first_ksteps(a.D) == 2) return launch_grad_d<MD, 0, 2>(critic, a, grid, s);
    return launch_grad_d<MD, 0, 8>(critic, a, grid, s);
}
int launch_td3_grad(bool critic, int md, const Td3GradArgs& a, int grid, hipStream_t s) {
    if (md == 256) return launch_grad<256>(critic, a, grid, s);
    if (md == 128) return launch_grad<128>(critic, a, grid, s);
    if (md == 64) return launch_grad<64>(critic, a, grid, s);
    set_error("no fused TD3 instantiation for width %d", md);
    return PIME_ERR_ARG;
}
int launch_td3_apply(const Td3ApplyArgs& a, hipStream_t s) {
    const int nwords = a.L.stride / 4;
    if (a.temp.alpha_log) hipLaunchKernelGGL(td3_apply_kernel<true>, dim3((nwords + kApplyWords - 1) / kApplyWords), dim3(kApplyThreads), 0, s, a);
    else hipLaunchKernelGGL(td3_apply_kernel<false>, dim3((nwords + kApplyWords - 1) / kApplyWords), dim3(kApplyThreads), 0, s, a);
    PIME_HIP_TRY(hipGetLastError());
    return PIME_OK;
}

}  // namespace pime
