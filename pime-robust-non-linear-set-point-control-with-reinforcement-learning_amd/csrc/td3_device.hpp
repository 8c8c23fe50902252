// Device code shared by the fused off-policy optimizer steps (td3_fused.hip, sac_fused.hip).  First the building blocks: the
// chain-layout activation images in LDS, the register-resident / streamed weight blocks, the layers on v_mfma_f32_16x16x4_f32, the
// weight-gradient slabs and the small-tensor images.  Then the pieces the four gradient kernels are made of -- the tile context, the
// minibatch gather, the twin target heads, the online twin-critic step, the target critic's forward and backward to the action, the
// actor body's backward -- and the host-side dispatch of (width, state width) to an instantiation.  What differs between the agents
// (the actors' forwards, the labels, the heads' gradients) is in their .hip files.  td3_fused.hip's header comment describes the
// decomposition all of this serves.
#pragma once
#include "td3.hpp"
#include "pime_common.hpp"

namespace pime {

typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int kTd3Tile = 16;
constexpr int kQP = 72, kTP = 4 * kQP;   // chain layout: floats between lane groups / tiles (72 = 16 samples x 4 + 8: the operand reads of the weight gradients hit 32 banks; pitches 68 .. 88 swept at the end of round 4: the launches take the same 20.0 / 21.7 us)
constexpr uint32_t STREAM_TD3_SMOOTH = 3;

#define TD3_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
#define TD3_NO_HOIST() asm volatile("" ::: "memory")

__device__ __forceinline__ f32x4_t mfma16(float a, float b, f32x4_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4_t ld4(const float* p) { return *reinterpret_cast<const f32x4_t*>(p); }
__device__ __forceinline__ void st4(float* p, const f32x4_t& v) { *reinterpret_cast<f32x4_t*>(p) = v; }
__device__ __forceinline__ f32x4_t relu4(f32x4_t v) {   // one v_med3_f32 per element (`v > 0 ? v : 0` compiles to a canonicalising max + a max)
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = __builtin_amdgcn_fmed3f(v[r], 0.f, __builtin_inff());
    return v;
}
// d * [h > 0] (torch's threshold_backward)
__device__ __forceinline__ f32x4_t gate4(f32x4_t d, const f32x4_t& h) {
#pragma unroll
    for (int r = 0; r < 4; ++r) d[r] = h[r] > 0.f ? d[r] : 0.f;
    return d;
}
template <int CTRL>
__device__ __forceinline__ float dpp_add16(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
// sum over the 16 lanes of a row (= the tile's 16 samples), result in every lane of the row; fixed order
__device__ __forceinline__ float row_sum16(float v) {
    v = dpp_add16<0xb1>(v);    // quad_perm [1,0,3,2]
    v = dpp_add16<0x4e>(v);    // quad_perm [2,3,0,1]
    v = dpp_add16<0x141>(v);   // row_half_mirror
    return dpp_add16<0x140>(v);   // row_mirror
}
__device__ __forceinline__ f32x4_t row_sum16(f32x4_t v) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = row_sum16(v[r]);
    return v;
}

// ---- chain-layout activation images in LDS ---------------------------------------------------------------------------------------
__device__ __forceinline__ void chain_put(float* __restrict__ buf, int lane, int tile, const f32x4_t& v) {
    st4(buf + tile * kTP + (lane >> 4) * kQP + (lane & 15) * 4, v);
}
template <int NT>
__device__ __forceinline__ void chain_get(const float* __restrict__ buf, int lane, f32x4_t (&v)[NT]) {
    const float* p = buf + (lane >> 4) * kQP + (lane & 15) * 4;
#pragma unroll
    for (int t = 0; t < NT; ++t) v[t] = ld4(p + t * kTP);
    // all NT reads are issued before the first MFMA that consumes one (left alone, hipcc re-uses the consumed weight registers as
    // destinations and issues the reads two at a time between the MFMAs: four exposed LDS round trips per layer); the counted
    // lgkmcnt waits are inserted after scheduling, so the MFMAs of k-tile t still wait for read t only
    __builtin_amdgcn_sched_barrier(0);
}
// element (feature 16 t + i, sample 4 s + q) of an image, for the lane (q, i): the A / B operand of a weight-gradient k-step
__device__ __forceinline__ float chain_elem(const float* __restrict__ buf, int lane, int t, int s) {
    const int i = lane & 15, q = lane >> 4;
    return buf[t * kTP + (i >> 2) * kQP + (4 * s + q) * 4 + (i & 3)];
}

// ---- weights: global -> registers --------------------------------------------------------------------------------------------------
// forward: A operand of output tile t0 + n, k-step (kt, r) = W[16 (t0 + n) + i][16 kt + 4 q + r]: component r of one 16-byte load
// (a wave-uniform base pointer + ONE 32-bit lane offset + compile-time offsets: with a 64-bit per-lane pointer hipcc spends two
// vector adds per load on the address; one wave per SIMD means every such instruction is exposed issue time)
template <int NT, int PER>
__device__ __forceinline__ void load_w(const float* __restrict__ W, int t0, int lane, f32x4_t (&w)[PER][NT]) {
    const int o = (16 * t0 + (lane & 15)) * (NT * 16) + 4 * (lane >> 4);
#pragma unroll
    for (int n = 0; n < PER; ++n)
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) w[n][kt] = ld4(W + o + n * 16 * (NT * 16) + 16 * kt);
}
// transposed (dX = W^T dZ): A operand of output (= input-feature) tile t0 + n, k-step (kt, r) = W[16 kt + 4 q + r][16 (t0 + n) + i]
template <int NT, int PER>
__device__ __forceinline__ void load_wt(const float* __restrict__ W, int t0, int lane, f32x4_t (&w)[PER][NT]) {
    const int o = (4 * (lane >> 4)) * (NT * 16) + 16 * t0 + (lane & 15);
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int n = 0; n < PER; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) w[n][kt][r] = W[o + (16 * kt + r) * (NT * 16) + 16 * n];
}

// Width 256 (NT = 16, eight waves, PER = 2): a [PER][NT] register block of one layer's weights is 128 VGPRs, two of them (the next
// layer's, loaded a layer ahead) plus the activation's in[NT] exceed the 256 VGPRs a wave has at two waves per SIMD.  There the
// weights are STREAMED: the layer walks its k-tiles in slices of kSliceK, the loads of slice c + 1 in flight while slice c's
// MFMAs issue (2 x PER x kSliceK x 4 = 64 VGPRs).  Wts<NT, PER, S> is what a wave holds between "load" and "layer": the registers
// (S = false: the round-4 code, unchanged) or just where the tensor is and whether it is read transposed (S = true).
constexpr int kSliceK = 4;
template <int NT, int PER, bool S>
struct Wts { f32x4_t w[PER][NT]; };
template <int NT, int PER>
struct Wts<NT, PER, true> { const float* W; bool tr; };

template <int NT, int PER>
__device__ __forceinline__ void wload(Wts<NT, PER, false>& w, const float* __restrict__ W, int t0, int lane) { load_w<NT, PER>(W, t0, lane, w.w); }
template <int NT, int PER>
__device__ __forceinline__ void wload_t(Wts<NT, PER, false>& w, const float* __restrict__ W, int t0, int lane) { load_wt<NT, PER>(W, t0, lane, w.w); }
template <int NT, int PER>
__device__ __forceinline__ void wload(Wts<NT, PER, true>& w, const float* W, int, int) { w.W = W; w.tr = false; }
template <int NT, int PER>
__device__ __forceinline__ void wload_t(Wts<NT, PER, true>& w, const float* W, int, int) { w.W = W; w.tr = true; }

// slice c of output tiles t0 .. t0 + PER - 1: k-tiles c kSliceK .. (c + 1) kSliceK - 1, as load_w / load_wt would hold them
template <int NT, int PER>
__device__ __forceinline__ void wslice(const float* __restrict__ W, bool tr, int t0, int lane, int c, f32x4_t (&w)[PER][kSliceK]) {
    constexpr int MD = NT * 16;
    if (!tr) {
        const int o = (16 * t0 + (lane & 15)) * MD + 4 * (lane >> 4);
#pragma unroll
        for (int n = 0; n < PER; ++n)
#pragma unroll
            for (int k = 0; k < kSliceK; ++k) w[n][k] = ld4(W + o + n * 16 * MD + 16 * (c * kSliceK + k));
    } else {
        const int o = (4 * (lane >> 4)) * MD + 16 * t0 + (lane & 15);
#pragma unroll
        for (int k = 0; k < kSliceK; ++k)
#pragma unroll
            for (int n = 0; n < PER; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r) w[n][k][r] = W[o + (16 * (c * kSliceK + k) + r) * MD + 16 * n];
    }
}

// out[n] += W in (output tiles t0 .. t0 + PER - 1).  The caller initialises out: bias_get IN FRONT of the barrier that publishes `in`
// (the bias lives in the small-tensor image; read behind the barrier it was the youngest LDS read in front of the first MFMA, which
// then waited for all of the activation's reads -- lgkmcnt(0) -- instead of the first), or zero4 for the backward chain.
template <int PER>
__device__ __forceinline__ void bias_get(const float* __restrict__ bias, int t0, int lane, f32x4_t (&out)[PER]) {
#pragma unroll
    for (int n = 0; n < PER; ++n) out[n] = ld4(bias + 16 * (t0 + n) + 4 * (lane >> 4));
}
template <int PER>
__device__ __forceinline__ void zero4(f32x4_t (&out)[PER]) {
#pragma unroll
    for (int n = 0; n < PER; ++n) out[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
}
template <int NT, int PER>
__device__ __forceinline__ void layer(const f32x4_t (&w)[PER][NT], const f32x4_t (&in)[NT], f32x4_t (&out)[PER]) {
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int n = 0; n < PER; ++n) out[n] = mfma16(w[n][kt][r], in[kt][r], out[n]);
}

template <int NT, int PER>
__device__ __forceinline__ void wlayer(const Wts<NT, PER, false>& w, const f32x4_t (&in)[NT], f32x4_t (&out)[PER]) { layer<NT, PER>(w.w, in, out); }
// the streamed layer: the same MFMAs in the same order as layer()
template <int NT, int PER>
__device__ __forceinline__ void wlayer(const Wts<NT, PER, true>& w, const f32x4_t (&in)[NT], f32x4_t (&out)[PER]) {
    static_assert(NT % kSliceK == 0, "whole k-slices");
    constexpr int NC = NT / kSliceK;
    const int lane = threadIdx.x & 63, t0 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * PER;
    f32x4_t buf[2][PER][kSliceK];
    wslice<NT, PER>(w.W, w.tr, t0, lane, 0, buf[0]);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        if (c + 1 < NC) wslice<NT, PER>(w.W, w.tr, t0, lane, c + 1, buf[(c + 1) & 1]);
#pragma unroll
        for (int k = 0; k < kSliceK; ++k)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int n = 0; n < PER; ++n) out[n] = mfma16(buf[c & 1][n][k][r], in[c * kSliceK + k][r], out[n]);
    }
}

// first layer, fan-in Din <= 4 KF: k-step k = input columns 4 k .. 4 k + 3.  x[k]: this lane's B operand of k-step k, input column
// 4 k + q of sample j (0 beyond Din).  W: the [md][Din] weights, in the small-tensor image or (width 256, KF = 8) in global memory.
template <int PER, int KF>
__device__ __forceinline__ void layer_first(const float* __restrict__ W, const float* __restrict__ bias, int Din, int t0, int lane,
                                            const float (&x)[KF], f32x4_t (&out)[PER]) {
    const int i = lane & 15, q = lane >> 4;
#pragma unroll
    for (int n = 0; n < PER; ++n) {
        const float* row = W + (size_t)(16 * (t0 + n) + i) * Din;
        float av[KF];
#pragma unroll
        for (int k = 0; k < KF; ++k) av[k] = 4 * k + q < Din ? row[4 * k + q] : 0.f;
        out[n] = ld4(bias + 16 * (t0 + n) + 4 * q);
#pragma unroll
        for (int k = 0; k < KF; ++k)
            if (k == 0 || Din > 4 * k) out[n] = mfma16(av[k], x[k], out[n]);
    }
}

// partial head: sum over this wave's PER * 16 features of w[f] h[j][f], for the lane's sample j (same value in the four lane groups)
template <int PER>
__device__ __forceinline__ float head_partial(const float* __restrict__ w, int t0, int lane, const f32x4_t (&h)[PER]) {
    float p = 0.f;
#pragma unroll
    for (int n = 0; n < PER; ++n) {
        const f32x4_t wv = ld4(w + 16 * (t0 + n) + 4 * (lane >> 4));
#pragma unroll
        for (int r = 0; r < 4; ++r) p = fmaf(h[n][r], wv[r], p);
    }
    p += __shfl_xor(p, 16);
    p += __shfl_xor(p, 32);
    return p;
}
// cross-wave sums through LDS: slot = kRedSlot floats [wave][sample] (up to eight waves), summed in wave order
constexpr int kRedSlot = 128;
__device__ __forceinline__ void red_put(float* __restrict__ red, int slot, int wave, int lane, float p) {
    if (lane < 16) red[slot * kRedSlot + wave * 16 + lane] = p;
}
template <int NW>
__device__ __forceinline__ float red_get(const float* __restrict__ red, int slot, int lane) {
    const float* p = red + slot * kRedSlot + (lane & 15);
    float s = p[0] + p[16];
#pragma unroll
    for (int w = 2; w < NW; ++w) s += p[16 * w];
    return s;
}

// ---- weight gradients ----------------------------------------------------------------------------------------------------------------
// acc[n][b] = sum over the tile's samples of dZ[s][16 (t0 + n) + .] (x) H[s][16 b + .]   (both operands from chain images)
template <int NT, int PER>
__device__ __forceinline__ void dw_blocks(const float* __restrict__ dz, const float* __restrict__ h, int t0, int lane,
                                          f32x4_t (&acc)[PER][NT]) {
#pragma unroll
    for (int n = 0; n < PER; ++n)
#pragma unroll
        for (int b = 0; b < NT; ++b) acc[n][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        float av[PER], bv[NT];
#pragma unroll
        for (int n = 0; n < PER; ++n) av[n] = chain_elem(dz, lane, t0 + n, s);
#pragma unroll
        for (int b = 0; b < NT; ++b) bv[b] = chain_elem(h, lane, b, s);
#pragma unroll
        for (int n = 0; n < PER; ++n)
#pragma unroll
            for (int b = 0; b < NT; ++b) acc[n][b] = mfma16(av[n], bv[b], acc[n][b]);
    }
}
// first-layer weight gradient: B = the tile's input rows [16 samples][XW columns, zero beyond Din] (xin), XW / 16 column tiles
template <int PER, int XW>
__device__ __forceinline__ void dw_first(const float* __restrict__ dz, const float* __restrict__ xin, int t0, int lane,
                                         f32x4_t (&acc)[PER][XW / 16]) {
    constexpr int CT = XW / 16;
#pragma unroll
    for (int n = 0; n < PER; ++n)
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[n][c] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        float bv[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) bv[c] = xin[(4 * s + (lane >> 4)) * XW + 16 * c + (lane & 15)];
#pragma unroll
        for (int n = 0; n < PER; ++n) {
            const float av = chain_elem(dz, lane, t0 + n, s);
#pragma unroll
            for (int c = 0; c < CT; ++c) acc[n][c] = mfma16(av, bv[c], acc[n][c]);
        }
    }
}
__device__ __forceinline__ void slab_put(float* __restrict__ p, f32x4_t v, bool accum) {
    if (accum) v += ld4(p);
    st4(p, v);
}
// a finished weight-gradient job -> the slab, block-major (one 16-byte store per lane and block).  The accumulate / overwrite decision
// (a later sample group of the same workgroup: batches beyond 512 tiles) is taken once per job, not per block.
template <int NT, int PER>
__device__ __forceinline__ void slab_blocks(float* __restrict__ seg, int t0, int lane, const f32x4_t (&acc)[PER][NT], bool accum) {
    float* const p = seg + (t0 * NT * 64 + lane) * 4;
    if (!accum) {
#pragma unroll
        for (int n = 0; n < PER; ++n)
#pragma unroll
            for (int b = 0; b < NT; ++b) st4(p + (n * NT + b) * 256, acc[n][b]);
    } else {
#pragma unroll
        for (int n = 0; n < PER; ++n)
#pragma unroll
            for (int b = 0; b < NT; ++b) st4(p + (n * NT + b) * 256, acc[n][b] + ld4(p + (n * NT + b) * 256));
    }
}
// width 256: dw_blocks + slab_blocks in column slices of BC blocks (acc[PER][NT] alone would be 128 VGPRs); every block is the
// same 4-k-step sum as in dw_blocks
template <int NT, int PER, int BC>
__device__ __forceinline__ void dw_slab_sliced(const float* __restrict__ dz, const float* __restrict__ h, float* __restrict__ seg, int t0,
                                               int lane, bool accum) {
    float* const p = seg + (t0 * NT * 64 + lane) * 4;
#pragma unroll
    for (int cb = 0; cb < NT; cb += BC) {
        f32x4_t acc[PER][BC];
#pragma unroll
        for (int n = 0; n < PER; ++n)
#pragma unroll
            for (int b = 0; b < BC; ++b) acc[n][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float av[PER], bv[BC];
#pragma unroll
            for (int n = 0; n < PER; ++n) av[n] = chain_elem(dz, lane, t0 + n, s);
#pragma unroll
            for (int b = 0; b < BC; ++b) bv[b] = chain_elem(h, lane, cb + b, s);
#pragma unroll
            for (int n = 0; n < PER; ++n)
#pragma unroll
                for (int b = 0; b < BC; ++b) acc[n][b] = mfma16(av[n], bv[b], acc[n][b]);
        }
#pragma unroll
        for (int n = 0; n < PER; ++n)
#pragma unroll
            for (int b = 0; b < BC; ++b) slab_put(p + (n * NT + cb + b) * 256, acc[n][b], accum);
    }
}
// weight gradient of an md x md layer into its slab segment: register-blocked (width <= 128, the round-4 code) or sliced (width 256)
template <int NT, int PER, bool S>
__device__ __forceinline__ void dw_slab(const float* __restrict__ dz, const float* __restrict__ h, float* __restrict__ seg, int t0, int lane,
                                        bool accum) {
    if constexpr (S) {
        dw_slab_sliced<NT, PER, 8>(dz, h, seg, t0, lane, accum);
    } else {
        f32x4_t acc[PER][NT];
        dw_blocks<NT, PER>(dz, h, t0, lane, acc);
        slab_blocks<NT, PER>(seg, t0, lane, acc, accum);
    }
}
// a vector gradient (bias, head weights) of this wave's features: v = per-sample terms, summed over the tile's samples
template <int PER>
__device__ __forceinline__ void vec_grad(float* __restrict__ seg, int t0, int lane, const f32x4_t (&v)[PER], bool accum) {
#pragma unroll
    for (int n = 0; n < PER; ++n) {
        const f32x4_t s = row_sum16(v[n]);
        if ((lane & 15) == 0) slab_put(seg + 16 * (t0 + n) + 4 * (lane >> 4), s, accum);
    }
}

// The SMALL tensors of a net -- first-layer weights, biases, heads: everything but the md x md matrices -- are read by every wave at
// the moment a layer starts; from global memory each such read is an exposed L2 round trip on the workgroup's critical path (a dozen
// per kernel).  They are copied into LDS once per workgroup, behind the minibatch gather: the flat tensors minus the big matrices,
// in the same order (td3.hpp), so that a small-image offset is the flat offset minus the matrices in front of it.
// Width 256 with the Stacking observations (KF = 8) leaves the first-layer weights in global memory: the four chain images take 72 KB
// there and the three nets' first layers (~8 k floats each at D = 30) another 96 KB, over the 160 KB of a compute unit.  The small
// image then starts at the first bias (W1 = 0, unused).
__host__ __device__ constexpr bool td3_w1_global(int D, int md) { return md == 256 && td3_first_ksteps(D) == 8; }
struct Td3SmallActor { int W1, b1, b2, b3, w4, b4, total; };
struct Td3SmallCritic { int W1, b1, b2, q1w, q1b, q2w, q2b, total; };
__host__ __device__ inline Td3SmallActor td3_small_actor(int D, int md) {
    const Td3ActorOff P = td3_actor_off(D, md);
    const int mm = md * md, s = td3_w1_global(D, md) ? P.b1 : 0;
    return Td3SmallActor{P.W1, P.b1 - s, P.b2 - mm - s, P.b3 - 2 * mm - s, P.w4 - 2 * mm - s, P.b4 - 2 * mm - s, P.total - 2 * mm - s};
}
__host__ __device__ inline Td3SmallCritic td3_small_critic(int D, int md) {
    const Td3CriticOff P = td3_critic_off(D, md);
    const int mm = md * md, s = td3_w1_global(D, md) ? P.b1 : 0;
    return Td3SmallCritic{P.W1, P.b1 - s, P.b2 - mm - s, P.q1w - mm - s, P.q1b - mm - s, P.q2w - mm - s, P.q2b - mm - s, P.total - mm - s};
}

struct Td3Lds {
    int buf[4], xin, red, small[3], total;
};
__host__ __device__ constexpr int td3_buf_floats(int NT) { return NT * kTP; }
// the tile's input rows in LDS: [16 samples][XW columns], XW = 16 (KF = 2) or 32 (KF = 8)
__host__ __device__ constexpr int td3_xin_width(int D) { return 16 * td3_first_tiles(D); }
// sa: floats of the actor's small image (td3_small_actor / sac_small_actor: the one size in which the two agents' maps differ)
__host__ __device__ inline Td3Lds td3_lds(int NT, int D, int sa) {
    Td3Lds L{};
    int o = 0;
    for (int k = 0; k < 4; ++k) { L.buf[k] = o; o += td3_buf_floats(NT); }
    L.xin = o; o += 16 * td3_xin_width(D);
    L.red = o; o += 8 * kRedSlot;
    const int sc = td3_small_critic(D, NT * 16).total;
    L.small[0] = o; o += sa;                 // the launch's actor (TD3's critic launch: the target actor)
    L.small[1] = o; o += sc;                 // the launch's critic (critic launch: the online critic; actor launch: the target critic)
    L.small[2] = o; o += sc;                 // critic launch only: the target critic
    L.total = o;
    return L;
}
__host__ __device__ inline Td3Lds td3_lds(int NT, int D) { return td3_lds(NT, D, td3_small_actor(D, NT * 16).total); }

// up to 256 16-byte words of a flat tensor, this thread's share: loaded here, written to LDS by small_store (the caller puts other
// loads in between, so that one memory round trip covers them all)
__device__ __forceinline__ f32x4_t small_load(const float* __restrict__ src, int n4, int tid) {
    return tid < n4 ? ld4(src + 4 * tid) : f32x4_t{0.f, 0.f, 0.f, 0.f};
}
__device__ __forceinline__ void small_store(float* __restrict__ dst, int n4, int tid, const f32x4_t& v) {
    if (tid < n4) st4(dst + 4 * tid, v);
}

// the generic staging of the Stacking / width-256 instantiations: floats [lo, hi) of a flat tensor to the small image (16-byte words,
// every thread of the workgroup taking words tid, tid + NTH, ...)
template <int NTH>
__device__ __forceinline__ void small_copy(float* __restrict__ dst, const float* __restrict__ src, int lo, int hi, int tid) {
    for (int u = tid; u < (hi - lo) / 4; u += NTH) st4(dst + 4 * u, ld4(src + lo + 4 * u));
}
// a whole net's small image that way, from flat float `lo` on (its W1, or b1 where td3_w1_global).  P / I: the net's flat and
// small-image offsets (Td3ActorOff / Td3SmallActor, SacActorOff / SacSmallActor: three runs around the two md x md matrices)
template <int NTH, class Off, class Img>
__device__ __forceinline__ void small_copy_actor(float* img, const float* src, int lo, const Off& P, const Img& I, int tid) {
    small_copy<NTH>(img, src, lo, P.W2, tid);
    small_copy<NTH>(img + I.b2, src, P.b2, P.W3, tid);
    small_copy<NTH>(img + I.b3, src, P.b3, P.total, tid);
}
template <int NTH>
__device__ __forceinline__ void small_copy_critic(float* img, const float* src, int lo, const Td3CriticOff& P, const Td3SmallCritic& I, int tid) {
    small_copy<NTH>(img, src, lo, P.W2, tid);
    small_copy<NTH>(img + I.b2, src, P.b2, P.total, tid);
}

// a standard normal draw of the optimizer steps: Philox4x32-10 keyed by seed, counter (batch position, epoch, table row, stream)
__device__ __forceinline__ float philox_normal_f32(uint64_t seed, uint32_t pos, uint32_t epoch, uint32_t trow, uint32_t stream) {
    double ua, ub;
    philox_pair(seed, pos, epoch, trow, stream, ua, ub);
    // Box-Muller (cosine branch) in float32 on the hardware transcendentals: the float64 log / sqrt / cos of the exploration kernels
    // are several hundred instructions, exposed issue time in front of this kernel's first barrier (1 - ua in (0, 1]: log finite)
    const float rad = __builtin_sqrtf(-2.0f * __logf((float)(1.0 - ua)));
    return rad * __cosf(6.2831853071795864769f * (float)ub);
}
// this lane's smoothing-noise draw for batch position pos
__device__ __forceinline__ float td3_noise(const Td3Batch& b, long long trow, int pos) {
    if (b.noise) return b.noise[(size_t)trow * b.B + pos];
    const uint32_t epoch = b.noise_epoch + (b.epoch ? (uint32_t)b.epoch[0] : 0u);   // bumped by the host per update
    return philox_normal_f32(b.noise_seed, (uint32_t)pos, epoch, (uint32_t)trow, STREAM_TD3_SMOOTH);
}

// ==== the pieces the four gradient kernels (td3_critic / td3_actor / sac_critic / sac_actor) are made of ===========================
// Each piece is a stretch of a kernel's group iteration, inlined where it is called.  The kernels' schedule lives in them: a piece
// takes the weights to prefetch as arguments and issues the load where the stretch always had it (a layer ahead of its use, in front
// of a barrier); its barriers are the kernel's barriers.  Common arguments: wave, t0 = the wave's first output tile, T = the tile
// context; B0 .. B3 = chain images, red = the reduction slots, sl / SL = the workgroup's slab and its layout; wA / wB = the two
// weight blocks a wave holds; in = the activation's B operands (scratch registers of the caller).

// ---- tile context: what a lane is in this group iteration ---------------------------------------------------------------------------
struct Td3Tile {
    int lane, j, q;   // lane of the wave = (lane group q, sample j of the tile)
    int pos, p;       // the sample's batch position, and the position it reads (the last row's where the tile runs past the batch)
    bool accum;       // a later group of this workgroup: the slab accumulates
    bool valid;       // pos < B
};
__device__ __forceinline__ Td3Tile td3_tile(int tid, int group, int B) {
    int lane = tid & 63;
    asm volatile("" : "+v"(lane));   // opaque per iteration: nothing derived from the lane is kept live across the group loop
    const int pos = group * kTd3Tile + (lane & 15);
    const bool valid = pos < B;
    return Td3Tile{lane, lane & 15, lane >> 4, pos, valid ? pos : B - 1, group != (int)blockIdx.x, valid};
}
// the workgroup's sums over its samples (wave 0, lanes 0..15 hold the terms) -> the slab's scalar slot, words [0 .. N)
template <int N>
__device__ __forceinline__ void tile_scalars_put(float* slot, int wave, int tid, const float (&acc)[N]) {
    static_assert(N <= 4, "the scalar slot is one 16-byte word");
    if (wave == 0) {
        f32x4_t v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int n = 0; n < N; ++n) v[n] = row_sum16(acc[n]);
        if (tid == 0) st4(slot, v);
    }
}

// ---- minibatch gather -------------------------------------------------------------------------------------------------------------------
// first-layer B operands of a critic on [s, act, 0 ..]: column 4 k + q of the lane's sample
template <int KF>
__device__ __forceinline__ void critic_input(const float (&s)[KF], float act, int D, int q, float (&x)[KF]) {
#pragma unroll
    for (int k = 0; k < KF; ++k) x[k] = 4 * k + q < D ? s[k] : (4 * k + q == D ? act : 0.f);
}
// wave 0: the tile's input rows [16 samples][XW columns, zero beyond 4 KF] for a first-layer weight gradient
template <int KF, int XW>
__device__ __forceinline__ void xin_put(float* xin, const Td3Tile& T, const float (&x)[KF]) {
#pragma unroll
    for (int k = 0; k < XW / 4; ++k) xin[T.j * XW + 4 * k + T.q] = k < KF ? x[k] : 0.f;
}
// The critic launch's gather in its three steps -- index, rows, publish -- between which the kernel issues its first weight load,
// stages the small tensors, draws its noise and passes the group's first barrier.  Batch: Td3Batch | SacBatch.
template <int KF>
struct Td3Gather {
    long long row, nrow;
    float sx[KF], nx[KF];          // state / next-state columns 4 k + q of the lane's sample (0 beyond D)
    float reward, mask, action;
    float xs[KF];                  // the online critic's input [s, a, 0 ..] (gather_publish)
};
template <int KF, class Batch>
__device__ __forceinline__ void gather_index(Td3Gather<KF>& G, const Batch& b, const Td3Tile& T) {
    G.row = b.idx[(size_t)b.row * b.B + T.p];
    G.nrow = b.nxt[(size_t)b.row * b.B + T.p];
}
template <int KF, class Batch>
__device__ __forceinline__ void gather_rows(Td3Gather<KF>& G, const Batch& b, int D, const Td3Tile& T) {
    const float* srow = b.state + (size_t)G.row * D;
    const float* nsrow = b.state + (size_t)G.nrow * D;
#pragma unroll
    for (int k = 0; k < KF; ++k) {
        G.sx[k] = 4 * k + T.q < D ? srow[4 * k + T.q] : 0.f;
        G.nx[k] = 4 * k + T.q < D ? nsrow[4 * k + T.q] : 0.f;
    }
    const float* orow = b.other + (size_t)G.row * 3;
    G.reward = orow[0]; G.mask = orow[1]; G.action = orow[2];
}
// behind the group's first barrier: xs, and by wave 0 the rows for the first-layer weight gradient (xin) and for the actor launch (xg)
template <int KF, int XW>
__device__ __forceinline__ void gather_publish(Td3Gather<KF>& G, int D, const Td3Tile& T, int wave, float* xin, float* xg) {
    critic_input<KF>(G.sx, G.action, D, T.q, G.xs);
    if (wave == 0) {
        xin_put<KF, XW>(xin, T, G.xs);
        if (T.valid) {
#pragma unroll
            for (int k = 0; k < KF; ++k) xg[(size_t)T.pos * (4 * KF) + 4 * k + T.q] = G.xs[k];
        }
    }
}
// the actor launch: the state rows as the critic launch of this step gathered them (one round trip instead of index -> row)
template <int KF>
__device__ __forceinline__ void gather_read(const float* xg, int D, const Td3Tile& T, float (&sx)[KF]) {
#pragma unroll
    for (int k = 0; k < KF; ++k) sx[k] = 4 * k + T.q < D ? xg[(size_t)T.p * (4 * KF) + 4 * k + T.q] : 0.f;
}

// ---- CriticTwin ---------------------------------------------------------------------------------------------------------------------------
// Twin heads of the critic whose small image is ct (first layer W1: there, or in global memory) on the prepared first-layer operand
// xt: the lane's sample's q1, q2.  wA holds its W2.  h1 passes through `img`; reduction slots slot, slot + 1.  Ends behind a barrier.
template <int NT, int PER, int NW, int KF, bool S>
__device__ __forceinline__ void twin_heads(const float* W1, const float* ct, const Td3SmallCritic& SC, int Dc, float* img, float* red, int slot,
                                           int wave, int t0, int lane, const float (&xt)[KF], const Wts<NT, PER, S>& wA, f32x4_t (&in)[NT],
                                           float& tq1, float& tq2) {
    f32x4_t h[PER];
    layer_first<PER, KF>(W1, ct + SC.b1, Dc, t0, lane, xt, h);
#pragma unroll
    for (int n = 0; n < PER; ++n) chain_put(img, lane, t0 + n, relu4(h[n]));
    bias_get<PER>(ct + SC.b2, t0, lane, h);
    TD3_BARRIER();
    chain_get<NT>(img, lane, in);
    wlayer(wA, in, h);
#pragma unroll
    for (int n = 0; n < PER; ++n) h[n] = relu4(h[n]);
    red_put(red, slot, wave, lane, head_partial<PER>(ct + SC.q1w, t0, lane, h));
    red_put(red, slot + 1, wave, lane, head_partial<PER>(ct + SC.q2w, t0, lane, h));
    TD3_BARRIER();
    tq1 = red_get<NW>(red, slot, lane) + ct[SC.q1b];
    tq2 = red_get<NW>(red, slot + 1, lane) + ct[SC.q2b];
}

// The online twin critic (small image cr, first layer W1, md x md weights W2 in global memory) on (s, a) = xs against `label`:
// forward, SmoothL1 x 2 (beta = 1, mean) and its gradient, backward, every weight gradient into the slab; the loss terms add to
// loss_acc (wave 0, lanes 0..15).  wB holds W2 on entry; W2^T is loaded into wA here.  h1 in B1, dZ2 in B2, dZ1 in B0; reduction
// slots slot, slot + 1; xin as gather_publish left it.
template <int NT, int PER, int NW, int KF, int XW, bool S>
__device__ __forceinline__ void online_critic_step(const float* W1, const float* cr, const Td3SmallCritic& SC, const float* W2, int Dc, float* B0,
                                                   float* B1, float* B2, const float* xin, float* red, int slot, int wave, int t0,
                                                   const Td3Tile& T, const float (&xs)[KF], float label, float invB, Wts<NT, PER, S>& wA,
                                                   const Wts<NT, PER, S>& wB, f32x4_t (&in)[NT], float* sl, const Td3SlabLayout& SL,
                                                   float& loss_acc) {
    constexpr int CT = XW / 16;
    const int lane = T.lane, q = T.q;
    const bool accum = T.accum;
    // ------------------------------------------------------------------ forward
    f32x4_t h1[PER], h2[PER];
    {
        layer_first<PER, KF>(W1, cr + SC.b1, Dc, t0, lane, xs, h1);
#pragma unroll
        for (int n = 0; n < PER; ++n) { h1[n] = relu4(h1[n]); chain_put(B1, lane, t0 + n, h1[n]); }
    }
    wload_t(wA, W2, t0, lane);   // for dH1 = W2^T dZ2
    bias_get<PER>(cr + SC.b2, t0, lane, h2);
    TD3_BARRIER();
    chain_get<NT>(B1, lane, in);
    wlayer(wB, in, h2);
#pragma unroll
    for (int n = 0; n < PER; ++n) h2[n] = relu4(h2[n]);
    red_put(red, slot, wave, lane, head_partial<PER>(cr + SC.q1w, t0, lane, h2));
    red_put(red, slot + 1, wave, lane, head_partial<PER>(cr + SC.q2w, t0, lane, h2));
    TD3_BARRIER();
    // ------------------------------------------------------------------ SmoothL1 x 2 (beta = 1, mean) and its gradient
    float g1 = 0.f, g2 = 0.f;
    {
        const float d1 = red_get<NW>(red, slot, lane) + cr[SC.q1b] - label, d2 = red_get<NW>(red, slot + 1, lane) + cr[SC.q2b] - label;
        const float a1 = fabsf(d1), a2 = fabsf(d2);
        if (T.valid) {
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

// The target critic on (s, a_policy) = xt in the actor launches, keeping c1 = relu(z1) (also in `img`) and c2 = relu(z2) for the
// backward.  wA holds its W2 on entry; W2^T is loaded into wB here.  The caller reduces the head(s) it needs from c2, writes the
// seed of the backward -- dZc2 = d obj / d q * w_head [c2 > 0] -- to a chain image and passes a barrier; then:
template <int NT, int PER, int KF, bool S>
__device__ __forceinline__ void target_critic_fwd(const float* W1, const float* ct, const Td3SmallCritic& SC, const float* W2, int Dc, float* img,
                                                  int t0, int lane, const float (&xt)[KF], const Wts<NT, PER, S>& wA, Wts<NT, PER, S>& wB,
                                                  f32x4_t (&in)[NT], f32x4_t (&c1)[PER], f32x4_t (&c2)[PER]) {
    layer_first<PER, KF>(W1, ct + SC.b1, Dc, t0, lane, xt, c1);
#pragma unroll
    for (int n = 0; n < PER; ++n) { c1[n] = relu4(c1[n]); chain_put(img, lane, t0 + n, c1[n]); }
    wload_t(wB, W2, t0, lane);   // dC1 = W2^T dZc2
    bias_get<PER>(ct + SC.b2, t0, lane, c2);
    TD3_BARRIER();
    chain_get<NT>(img, lane, in);
    wlayer(wA, in, c2);
#pragma unroll
    for (int n = 0; n < PER; ++n) c2[n] = relu4(c2[n]);
}
// ... d obj / d action through the critic = sum_f W1[f][D] dZc1[f], dZc1 = (W2^T dZc2) [c1 > 0], from the seed in `seed` (wB: W2^T).
// Ends behind a barrier.
template <int NT, int PER, int NW, bool S>
__device__ __forceinline__ float critic_to_action(const float* W1, int D, const float* seed, float* red, int slot, int wave, int t0, int lane,
                                                  const Wts<NT, PER, S>& wB, f32x4_t (&in)[NT], const f32x4_t (&c1)[PER]) {
    const int q = lane >> 4, Dc = D + 1;
    chain_get<NT>(seed, lane, in);
    f32x4_t d[PER];
    zero4<PER>(d);
    wlayer(wB, in, d);
    float pa = 0.f;
#pragma unroll
    for (int n = 0; n < PER; ++n) {
        d[n] = gate4(d[n], c1[n]);
#pragma unroll
        for (int r = 0; r < 4; ++r) pa = fmaf(d[n][r], W1[(16 * (t0 + n) + 4 * q + r) * Dc + D], pa);
    }
    pa += __shfl_xor(pa, 16);
    pa += __shfl_xor(pa, 32);
    red_put(red, slot, wave, lane, pa);
    TD3_BARRIER();
    return red_get<NW>(red, slot, lane);
}

// ---- three-layer actor body: backward + weight gradients ------------------------------------------------------------------------------
// The gate of the two upper layers is the agent's: TD3's body is ReLU throughout (the gate reads the stored activations), SAC's upper
// layers are Hardswish (sac_fused.hip: the gate reads the stored pre-activations).  The first layer is ReLU in both.
struct GateRelu {
    static __device__ __forceinline__ f32x4_t bwd(const f32x4_t& d, const f32x4_t& h) { return gate4(d, h); }
};
// From the last hidden layer's dZ3 (the caller has put it in B2, with that layer's bias gradient and the heads' gradients in the slab)
// down to the first layer: slab segments 0 .. 4.  B0 / B1 hold the first / second layer's activations, xin the input rows; a1 = the
// first layer's activations, s2 = what Gate reads of the second layer.  wA holds W3^T on entry; W2^T is loaded into wB here.
template <class Gate, int NT, int PER, int XW, bool S>
__device__ __forceinline__ void actor_body_bwd(const float* W2, float* B0, float* B1, float* B2, float* B3, const float* xin, int t0,
                                               const Td3Tile& T, const Wts<NT, PER, S>& wA, Wts<NT, PER, S>& wB, f32x4_t (&in)[NT],
                                               const f32x4_t (&a1)[PER], const f32x4_t (&s2)[PER], float* sl, const Td3SlabLayout& SL) {
    constexpr int CT = XW / 16;
    const int lane = T.lane;
    const bool accum = T.accum;
    wload_t(wB, W2, t0, lane);   // dA1 = W2^T dZ2
    TD3_BARRIER();   // dZ3 published
    dw_slab<NT, PER, S>(B2, B1, sl + SL.seg[4].slab_off, t0, lane, accum);   // third layer: dZ3^T A2
    TD3_NO_HOIST();
    chain_get<NT>(B2, lane, in);
    {
        f32x4_t d[PER];
        zero4<PER>(d);
        wlayer(wA, in, d);
#pragma unroll
        for (int n = 0; n < PER; ++n) { d[n] = Gate::bwd(d[n], s2[n]); chain_put(B3, lane, t0 + n, d[n]); }
        vec_grad<PER>(sl + SL.seg[3].slab_off, t0, lane, d, accum);    // second layer's bias
    }
    TD3_BARRIER();   // dZ2 published
    dw_slab<NT, PER, S>(B3, B0, sl + SL.seg[2].slab_off, t0, lane, accum);   // second layer: dZ2^T A1
    TD3_NO_HOIST();
    chain_get<NT>(B3, lane, in);
    {
        f32x4_t d[PER];
        zero4<PER>(d);
        wlayer(wB, in, d);
#pragma unroll
        for (int n = 0; n < PER; ++n) { d[n] = gate4(d[n], a1[n]); chain_put(B1, lane, t0 + n, d[n]); }
        vec_grad<PER>(sl + SL.seg[1].slab_off, t0, lane, d, accum);    // first layer's bias
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

// ==== host side: one dispatch for both agents' gradient launches =====================================================================
// K names an agent's kernel pair: K::Args, K::serves<MD, KF>(), K::lds_floats(NT, D), K::critic<MD, DD, NW, KF>() / K::actor<...>()
// (the kernels).  The state width is compiled in for the environments' observations (3: pH, 4: water-tank Integrator, 12 / 30:
// water-tank Stacking4 / Stacking10), else read from the arguments.
// Waves per workgroup.  Width 64 has four output tiles: four waves, one per SIMD.  Widths 128 and 256: eight waves, two per SIMD,
// owning one / two of a layer's eight / sixteen output tiles (the non-MFMA instructions of one wave issue behind the other's MFMAs);
// at width 128 that measured 60.4 us per optimizer step against 63.1 on four waves (profiles/r04_u_td3_waves_ab.txt).
template <class K, int MD, int DD, int KF>
static int grad_launch(bool critic, const typename K::Args& a, int grid, hipStream_t s) {
    if constexpr (K::template serves<MD, KF>()) {
        constexpr int NW = MD == 64 ? 4 : 8;
        const size_t lds_bytes = sizeof(float) * (size_t)K::lds_floats(MD / 16, a.D);
        if (critic) hipLaunchKernelGGL((K::template critic<MD, DD, NW, KF>()), dim3(grid), dim3(NW * 64), lds_bytes, s, a);
        else hipLaunchKernelGGL((K::template actor<MD, DD, NW, KF>()), dim3(grid), dim3(NW * 64), lds_bytes, s, a);
        PIME_HIP_TRY(hipGetLastError());
        return PIME_OK;
    } else {
        // not reached while the callers refuse what K::serves refuses; says so if one of them is widened alone
        set_error("no fused instantiation for width %d with %d first-layer k-steps", MD, KF);
        return PIME_ERR_ARG;
    }
}
template <class K, int MD>
static int grad_dispatch_d(bool critic, const typename K::Args& a, int grid, hipStream_t s) {
    if (a.D == 3) return grad_launch<K, MD, 3, 2>(critic, a, grid, s);
    if (a.D == 4) return grad_launch<K, MD, 4, 2>(critic, a, grid, s);
    if (a.D == 12) return grad_launch<K, MD, 12, 8>(critic, a, grid, s);
    if (a.D == 30) return grad_launch<K, MD, 30, 8>(critic, a, grid, s);
    if (td3_first_ksteps(a.D) == 2) return grad_launch<K, MD, 0, 2>(critic, a, grid, s);
    return grad_launch<K, MD, 0, 8>(critic, a, grid, s);
}
template <class K>
static int grad_dispatch(bool critic, int md, const typename K::Args& a, int grid, hipStream_t s) {
    if (md == 256) return grad_dispatch_d<K, 256>(critic, a, grid, s);
    if (md == 128) return grad_dispatch_d<K, 128>(critic, a, grid, s);
    return grad_dispatch_d<K, 64>(critic, a, grid, s);
}

}  // namespace pime
