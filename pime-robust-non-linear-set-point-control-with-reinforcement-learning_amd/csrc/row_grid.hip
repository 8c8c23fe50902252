// The finishing launch of the row grid (row_grid.hpp): one kernel for every sweep on that tiling.
#include "row_grid.hpp"

namespace pime {

// summary[p][cell][:] from rows[cell][p][0 .. N): one wave per (p, cell), cell = seg * ROWS + metric row.  Lane l of block b holds
// plant 64 b + l (coalesced); the butterfly is SweepDeviceSink's (prior_sweep.hip), the blocks follow in ascending order.
__global__ __launch_bounds__(kRowGridThreads) void row_grid_finish_kernel(int P, int N, int cells, const double* __restrict__ rows,
                                                                          double* __restrict__ summary) {
    const int lane = threadIdx.x & 63;
    const long long wv = (long long)blockIdx.x * (kRowGridThreads / 64) + (threadIdx.x >> 6);
    if (wv >= (long long)P * cells) return;   // wave-uniform
    const int p = (int)(wv / cells), cell = (int)(wv - (long long)p * cells);
    const double* x = rows + ((size_t)cell * P + p) * N;
    double total = 0.0, mn_all = __builtin_huge_val(), mx_all = -__builtin_huge_val();
    int arg_all = -1, cnt_all = 0;
    for (int b = 0; b * kSweepBlockPlants < N; ++b) {
        const int i = b * kSweepBlockPlants + lane;
        const double v = i < N ? x[i] : 0.0;
        const bool c = i < N && sweep_counts(v);   // absent plants and uncounted values (a sweep's NaN rows among them): +0.0, +-inf, no index
        double s = c ? v : 0.0, mn = c ? v : __builtin_huge_val(), mx = c ? v : -__builtin_huge_val();
        int arg = c ? i : -1, cnt = c ? 1 : 0;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            s += __shfl_xor(s, off, 64);
            const double mo = __shfl_xor(mn, off, 64), xo = __shfl_xor(mx, off, 64);
            const int ao = __shfl_xor(arg, off, 64);
            cnt += __shfl_xor(cnt, off, 64);
            mn = mo < mn ? mo : mn;
            if (xo > mx || (xo == mx && ao < arg)) { mx = xo; arg = ao; }   // a tie: the smaller plant index
        }
        total = b == 0 ? s : total + s;
        mn_all = mn < mn_all ? mn : mn_all;
        if (b == 0 || mx > mx_all) { mx_all = mx; arg_all = arg; }   // strictly: a tie keeps the earlier block
        cnt_all += cnt;
    }
    if (lane == 0) {
        double* q = summary + ((size_t)p * cells + cell) * PIME_SWEEP_STATS;
        q[PIME_SWEEP_SUM] = total; q[PIME_SWEEP_MIN] = mn_all; q[PIME_SWEEP_MAX] = mx_all; q[PIME_SWEEP_ARGMAX] = (double)arg_all;
        q[PIME_SWEEP_FINITE] = (double)cnt_all;
    }
}

int launch_row_grid_finish(int P, int N, int cells, const double* rows, double* summary, hipStream_t stream) {
    const long long waves = (long long)P * cells;
    hipLaunchKernelGGL(row_grid_finish_kernel, dim3((unsigned)((waves + kRowGridThreads / 64 - 1) / (kRowGridThreads / 64))),
                       dim3(kRowGridThreads), 0, stream, P, N, cells, rows, summary);
    PIME_HIP_TRY(hipGetLastError());
    return PIME_OK;
}

}  // namespace pime
