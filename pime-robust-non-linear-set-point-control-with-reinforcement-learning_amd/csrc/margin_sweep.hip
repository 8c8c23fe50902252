// pime_margin_sweep: a grid of loop perturbations (gain, dead time, sensor noise) over the plants of a handle, on the row grid
// (row_grid.hpp has the tiling, the kernel and the launcher; margin_sweep.hpp the pair function).  A row decodes to g, d and sigma,
// wave-uniform: the delay line is read through a uniform switch, a row without noise skips the draw as a whole wave.
#include "margin_sweep.hpp"
#include "row_grid.hpp"

namespace pime {

struct MarginSweep {
    template <typename S>
    using Args = MarginArgs<S>;
    using Row = MarginRow;
    static constexpr int kCols = PIME_PERTURB_COLS, kRows = PIME_METRIC_ROWS;
    static constexpr const char* kNoun = "loop-perturbation";
    static __device__ __forceinline__ Row row(const double* r) { return margin_row(r); }

    struct Sink : RowGridSink {
        __device__ __forceinline__ void operator()(int seg, const SegMetrics& M) const {
            if (writer) {
                double v[kRows];
                sweep_rows(M, v);
                store(seg, v);
            }
        }
    };
    // gid, the PLANT's global lane, keys the measurement noise (and the tank's process noise).  nz is copied in front of the call:
    // the key is then read where a kernel that calls the pair function itself reads it, and the kernels keep their instructions
    template <typename S, typename Pol>
    static __device__ __forceinline__ void ph(const MarginArgs<S>& a, int i, const double (&K)[3], const Row& row, const Pol& pol, Sink& sink) {
        const uint32_t gid = a.env_offset + (uint32_t)i;
        PhLane<S> E{};
        ph_lane_load<S>(a.p, a.st, i, E);
        const MarginNoise nz = a.nz;
        margin_ph_pair<S>(a.p, a.st.table, gid, E, K, row, nz, a.s, pol, sink);
    }
    template <typename S, typename Pol>
    static __device__ __forceinline__ void wt(const MarginArgs<S>& a, int i, const double (&K)[4], const Row& row, const Pol& pol, Sink& sink) {
        const uint32_t gid = a.env_offset + (uint32_t)i;
        WtLane<S> W{};
        wt_lane_load<S>(a.wp, a.wst, i, W);
        const MarginNoise nz = a.nz;
        margin_wt_pair<S>(a.wp, gid, W, K, row, nz, a.s, pol, sink);
    }
};

template <typename S>
int launch_margin_sweep(int kind, int md, const MarginArgs<S>& a, const double* perturb, double* pairs, double* summary, double* actions,
                        double* outputs, double* workspace, hipStream_t stream) {
    return launch_row_grid<MarginSweep, S>(kind, md, a, perturb, pairs, summary, actions, outputs, workspace, stream);
}

template int launch_margin_sweep<double>(int, int, const MarginArgs<double>&, const double*, double*, double*, double*, double*, double*,
                                         hipStream_t);
template int launch_margin_sweep<float>(int, int, const MarginArgs<float>&, const double*, double*, double*, double*, double*, double*,
                                        hipStream_t);

}  // namespace pime
