// Launch-argument blocks and parameter / slab layouts of the fused SAC optimizer step (sac_fused.hip), shared with abi.hip.  The
// critic is TD3's CriticTwin (td3.hpp: td3_critic_off / td3_critic_slab); the apply launch is td3_apply_kernel.
#pragma once
#include "td3.hpp"

namespace pime {

constexpr int kSacMaxD = 7;   // the critic's D + 1 inputs fit 8 columns: first layers in two 16x16x4 k-steps (td3_first_ksteps)

// Flat parameter layout of ActorSAC (net.py:175-239), nn.Module parameter order, every tensor on a multiple of 4 floats, padding zero:
//   net_state.0.w [md][D], .b, net_state.2.w [md][md], .b, net_state.4.w [md][md], .b, net_a_avg.w [1][md], .b, net_a_std.w [1][md], .b
struct SacActorOff { int W1, b1, W2, b2, W3, b3, wa, ba, ws, bs, total; };
__host__ __device__ inline SacActorOff sac_actor_off(int D, int md) {
    SacActorOff o{};
    int p = 0;
    auto seg = [&](int& f, int n) { f = p; p = td3_align4(p + n); };
    seg(o.W1, md * D); seg(o.b1, md); seg(o.W2, md * md); seg(o.b2, md); seg(o.W3, md * md); seg(o.b3, md);
    seg(o.wa, md); seg(o.ba, 1); seg(o.ws, md); seg(o.bs, 1);
    o.total = p;
    return o;
}
// one workgroup's partial actor gradient (td3.hpp: Td3SlabLayout); scalar slot [0] = sum of min(q1, q2) + lp alpha
__host__ __device__ inline Td3SlabLayout sac_actor_slab(int D, int md) {
    const SacActorOff P = sac_actor_off(D, md);
    const int NT = md / 16;
    Td3SlabLayout L{};
    int o = 0, k = 0;
    auto mat = [&](int flat, int tb, int ldw) { L.seg[k++] = Td3Seg{o, NT * tb * 64, flat, tb, ldw, ldw, 0}; o += NT * tb * 256; };
    auto vec = [&](int flat, int n) { L.seg[k++] = Td3Seg{o, td3_align4(n) / 4, flat, 0, 0, 0, n}; o += td3_align4(n); };
    mat(P.W1, td3_first_tiles(D), D); vec(P.b1, md); mat(P.W2, NT, md); vec(P.b2, md); mat(P.W3, NT, md); vec(P.b3, md);
    vec(P.wa, md); vec(P.ba, 1); vec(P.ws, md); vec(P.bs, 1);
    L.nseg = k; L.scalar_off = o; L.stride = o + 4;
    return L;
}

struct SacBatch {
    const float* state;        // [rows][D] replay states
    const float* other;        // [rows][3]: reward * scale, mask (0 | gamma), action
    const int64_t* idx;        // [table rows][B] sampled rows; the successor state of row idx is row nxt
    const int64_t* nxt;
    const float* noise_next;   // [table rows][B] standard normal draws of a' (get_obj_critic_raw) / of a_pg, or NULL: Philox in the
    const float* noise_pg;     //   kernels, streams 4 / 5
    long long row;             // table row of this optimizer step (a launch argument)
    const int64_t* epoch;      // NULL, or [dev] int64[1] added to noise_epoch
    int B;
    uint64_t noise_seed;
    uint32_t noise_epoch;
};

struct SacGradArgs {
    SacBatch b;
    int D;
    const float* act;          // the ONLINE actor (both launches: SAC has no actor target)
    const float* cri;          // critic launch: the ONLINE critic;  actor launch: the TARGET critic (after the step's soft update)
    const float* cri_target;   // critic launch only
    const float* alpha_log;    // [dev] float32[1]: read at launch start (actor launch: after the temperature's step)
    float* slab;               // [grid][stride]
    float* xg;                 // [B][8]: the minibatch's state rows (+ action), gathered by the critic launch, read by the actor launch
    int stride, ngroups;
};

// sac_fused.hip, host side
bool sac_supported(int D, int action_dim, int md);
int64_t sac_workspace_floats(int D, int md, int B);     // both nets' slabs + the gathered rows
int launch_sac_grad(bool critic, int md, const SacGradArgs& a, int grid, hipStream_t s);

}  // namespace pime
