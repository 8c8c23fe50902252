// Device code shared by the fused off-policy optimizer steps (td3_fused.hip, sac_fused.hip): the chain-layout activation images in
// LDS, the register-resident / streamed weight blocks, the layers on v_mfma_f32_16x16x4_f32, the weight-gradient slabs and the
// small-tensor images.  td3_fused.hip's header comment describes the decomposition these pieces serve.
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
__host__ __device__ inline Td3Lds td3_lds(int NT, int D) {
    Td3Lds L{};
    int o = 0;
    for (int k = 0; k < 4; ++k) { L.buf[k] = o; o += td3_buf_floats(NT); }
    L.xin = o; o += 16 * td3_xin_width(D);
    L.red = o; o += 8 * kRedSlot;
    const int md = NT * 16, sa = td3_small_actor(D, md).total, sc = td3_small_critic(D, md).total;
    L.small[0] = o; o += sa;                 // the launch's actor (critic launch: the target actor)
    L.small[1] = o; o += sc;                 // the launch's critic (critic launch: the online critic; actor launch: the target critic)
    L.small[2] = o; o += sc;                 // critic launch only: the target critic
    L.total = o;
    return L;
}

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

}  // namespace pime
