// pime_actuator_sweep: a grid of actuator and sensor limits (saturation, slew rate, dead-band, DAC and ADC quanta) over the plants of
// a handle, on the row grid (row_grid.hpp has the tiling, the kernel and the launcher; actuator_sweep.hpp the pair function).  A row
// decodes to the six columns and one flag per stage, wave-uniform: every "is this stage on" is a uniform branch.  A pair stores sixteen
// rows per segment.  The row grid carries two traces; the third (`commands`) travels in the argument block and is stored under the
// sink's writer and column.
#include "actuator_sweep.hpp"
#include "row_grid.hpp"

namespace pime {

struct ActuatorSweep {
    template <typename S>
    using Args = ActArgs<S>;
    using Row = ActRow;
    static constexpr int kCols = PIME_ACT_COLS, kRows = kActAllRows;
    static constexpr const char* kNoun = "actuator-limits";
    static __device__ __forceinline__ Row row(const double* r) { return act_row(r); }

    struct Sink : RowGridSink {
        double* __restrict__ commands;   // [n_steps][P * N] or nullptr
        __device__ __forceinline__ void command(int t, double a_c) const {
            if (writer && commands != nullptr) commands[(size_t)t * PN + col] = a_c;
        }
        __device__ __forceinline__ void operator()(int seg, const SegMetrics& M, const ActMetrics& Q) const {
            if (writer) {
                double v[kRows];
                act_rows(M, Q, v);
                store(seg, v);
            }
        }
    };
    template <typename S, typename Pol>
    static __device__ __forceinline__ void ph(const ActArgs<S>& a, int i, const double (&K)[3], const Row& row, const Pol& pol, Sink& sink) {
        sink.commands = a.commands;
        PhLane<S> E{};
        ph_lane_load<S>(a.p, a.st, i, E);
        act_ph_pair<S>(a.p, a.st.table, E, K, row, a.s, pol, sink);
    }
    // gid, the PLANT's global lane, keys the tank's process noise
    template <typename S, typename Pol>
    static __device__ __forceinline__ void wt(const ActArgs<S>& a, int i, const double (&K)[4], const Row& row, const Pol& pol, Sink& sink) {
        sink.commands = a.commands;
        const uint32_t gid = a.env_offset + (uint32_t)i;
        WtLane<S> W{};
        wt_lane_load<S>(a.wp, a.wst, i, W);
        act_wt_pair<S>(a.wp, gid, W, K, row, a.s, pol, sink);
    }
};

template <typename S>
int launch_actuator_sweep(int kind, int md, const ActArgs<S>& a, const double* actuator, double* pairs, double* summary, double* actions,
                          double* outputs, double* workspace, hipStream_t stream) {
    return launch_row_grid<ActuatorSweep, S>(kind, md, a, actuator, pairs, summary, actions, outputs, workspace, stream);
}

template int launch_actuator_sweep<double>(int, int, const ActArgs<double>&, const double*, double*, double*, double*, double*, double*,
                                           hipStream_t);
template int launch_actuator_sweep<float>(int, int, const ActArgs<float>&, const double*, double*, double*, double*, double*, double*,
                                          hipStream_t);

}  // namespace pime
