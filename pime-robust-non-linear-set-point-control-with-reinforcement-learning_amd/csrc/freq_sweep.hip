// pime_freq_sweep: a grid of sinusoidal (or any tabulated) excitations -- at the set-point, in front of the actuator, on the
// measurement -- over the plants of a handle, on the row grid (row_grid.hpp has the tiling, the kernel and the launcher; freq_sweep.hpp
// the pair function).  A row decodes to the injection point, the amplitude and the window's onset, wave-uniform, and so is the row's
// table: a step reads its (c_k, s_k) through one uniform 16-byte load.  A pair stores sixteen rows per segment.
#include "freq_sweep.hpp"
#include "row_grid.hpp"

namespace pime {

struct FreqSweep {
    template <typename S>
    using Args = FreqArgs<S>;
    using Row = FreqRow;
    static constexpr int kCols = PIME_FREQ_COLS, kRows = kFreqAllRows;
    static constexpr const char* kNoun = "frequency-response";
    static __device__ __forceinline__ Row row(const double* r) { return freq_row(r); }

    struct Sink : RowGridSink {
        __device__ __forceinline__ void operator()(int seg, const SegMetrics& M, const FreqMetrics& Q) const {
            if (writer) {
                double v[kRows];
                freq_rows(M, Q, v);
                store(seg, v);
            }
        }
    };
    // the table of the wave's row: the sink's column is p * N + i and P * N < 2^31, so p is one 32-bit division per tile; every lane
    // of a wave holds the same p (row_grid.hpp), which readfirstlane tells the compiler
    template <typename S>
    static __device__ __forceinline__ const double* table(const FreqArgs<S>& a, int i, const Sink& sink) {
        const uint32_t p = (uint32_t)(sink.col - (size_t)i) / (uint32_t)a.n;
        return a.wave + (size_t)__builtin_amdgcn_readfirstlane((int)p) * (size_t)a.wave_len * 2;
    }
    template <typename S, typename Pol>
    static __device__ __forceinline__ void ph(const FreqArgs<S>& a, int i, const double (&K)[3], const Row& row, const Pol& pol, Sink& sink) {
        PhLane<S> E{};
        ph_lane_load<S>(a.p, a.st, i, E);
        freq_ph_pair<S>(a.p, a.st.table, E, K, row, table<S>(a, i, sink), a.s, pol, sink);
    }
    // gid, the PLANT's global lane, keys the tank's process noise
    template <typename S, typename Pol>
    static __device__ __forceinline__ void wt(const FreqArgs<S>& a, int i, const double (&K)[4], const Row& row, const Pol& pol, Sink& sink) {
        const uint32_t gid = a.env_offset + (uint32_t)i;
        WtLane<S> W{};
        wt_lane_load<S>(a.wp, a.wst, i, W);
        freq_wt_pair<S>(a.wp, gid, W, K, row, table<S>(a, i, sink), a.s, pol, sink);
    }
};

template <typename S>
int launch_freq_sweep(int kind, int md, const FreqArgs<S>& a, const double* excite, double* pairs, double* summary, double* actions,
                      double* outputs, double* workspace, hipStream_t stream) {
    return launch_row_grid<FreqSweep, S>(kind, md, a, excite, pairs, summary, actions, outputs, workspace, stream);
}

template int launch_freq_sweep<double>(int, int, const FreqArgs<double>&, const double*, double*, double*, double*, double*, double*,
                                       hipStream_t);
template int launch_freq_sweep<float>(int, int, const FreqArgs<float>&, const double*, double*, double*, double*, double*, double*,
                                      hipStream_t);

}  // namespace pime
