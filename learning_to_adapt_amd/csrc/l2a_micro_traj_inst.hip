// l2a_micro_traj_inst.hip - the trajectory-writing instances of the LSTM micro-tile kernel (l2a_lstm_micro_k<UW, true>,
// l2a_micro.h) as a translation unit of their own: l2a_micro_inst.hip keeps the instantiations it always had.
#include "l2a_micro.h"
#include "l2a_micro_launch.h"

namespace {

template <int UW>
int launch_traj(const L2ALstmParams* p, unsigned grid, int smem, hipStream_t stream) {
    auto kernel = l2a_lstm_micro_k<UW, true>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), smem, stream, *p);
    return 0;
}

}  // namespace

int l2a_launch_lstm_micro_traj(int units, const L2ALstmParams* p, unsigned grid, int smem, hipStream_t stream) {
    if (units == 256) return launch_traj<1>(p, grid, smem, stream);
    if (units == 512) return launch_traj<2>(p, grid, smem, stream);
    return -100;
}
