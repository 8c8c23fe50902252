// pime_disturb_sweep: a grid of disturbances (a load step at the plant input, a step of the plant parameters; a pulse of either)
// over the plants of a handle, on the row grid (row_grid.hpp has the tiling, the kernel and the launcher; disturb_sweep.hpp the pair
// function).  A row decodes to the onset, the length, the load and the multipliers, wave-uniform: "is the row active at step k" is a
// uniform branch, and so is the choice between the two plant sets a pair holds in registers.  A pair stores fifteen rows per segment.
#include "disturb_sweep.hpp"
#include "row_grid.hpp"

namespace pime {

struct DisturbSweep {
    template <typename S>
    using Args = DisturbArgs<S>;
    using Row = DisturbRow;
    static constexpr int kCols = PIME_DISTURB_COLS, kRows = kDisturbAllRows;
    static constexpr const char* kNoun = "disturbance-rejection";
    static __device__ __forceinline__ Row row(const double* r) { return disturb_row(r); }

    struct Sink : RowGridSink {
        __device__ __forceinline__ void operator()(int seg, const SegMetrics& M, const DistMetrics& Q) const {
            if (writer) {
                double v[kRows];
                disturb_rows(M, Q, v);
                store(seg, v);
            }
        }
    };
    template <typename S, typename Pol>
    static __device__ __forceinline__ void ph(const DisturbArgs<S>& a, int i, const double (&K)[3], const Row& row, const Pol& pol, Sink& sink) {
        PhLane<S> E{};
        ph_lane_load<S>(a.p, a.st, i, E);
        E.qww = a.st.qww[i]; E.qc = a.st.qc[i];   // (ph_lane_load zeroes them; the disturbed plant is rebuilt from the stored pair)
        disturb_ph_pair<S>(a.p, a.st.table, E, K, row, a.s, pol, sink);
    }
    // gid, the PLANT's global lane, keys the tank's process noise
    template <typename S, typename Pol>
    static __device__ __forceinline__ void wt(const DisturbArgs<S>& a, int i, const double (&K)[4], const Row& row, const Pol& pol, Sink& sink) {
        const uint32_t gid = a.env_offset + (uint32_t)i;
        WtLane<S> W{};
        wt_lane_load<S>(a.wp, a.wst, i, W);
        disturb_wt_pair<S>(a.wp, gid, W, K, row, a.s, pol, sink);
    }
};

template <typename S>
int launch_disturb_sweep(int kind, int md, const DisturbArgs<S>& a, const double* disturb, double* pairs, double* summary, double* actions,
                         double* outputs, double* workspace, hipStream_t stream) {
    return launch_row_grid<DisturbSweep, S>(kind, md, a, disturb, pairs, summary, actions, outputs, workspace, stream);
}

template int launch_disturb_sweep<double>(int, int, const DisturbArgs<double>&, const double*, double*, double*, double*, double*, double*,
                                          hipStream_t);
template int launch_disturb_sweep<float>(int, int, const DisturbArgs<float>&, const double*, double*, double*, double*, double*, double*,
                                         hipStream_t);

}  // namespace pime
