// l2a_mlp_micro_traj_inst.hip - the trajectory-writing instances of the MLP micro-tile kernel (l2a_mlp_micro_k<UW, GACT, true>,
// l2a_micro.h) as a translation unit of their own: l2a_micro_inst.hip keeps the instantiations it always had.
#include "l2a_micro.h"
#include "l2a_micro_launch.h"

namespace {

template <int UW, bool GACT>
int launch_traj(const L2AKParams* p, unsigned grid, int smem, hipStream_t stream) {
    auto kernel = l2a_mlp_micro_k<UW, GACT, true>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), smem, stream, *p);
    return 0;
}

}  // namespace

int l2a_launch_mlp_micro_traj(int hidden, int gact, const L2AKParams* p, unsigned grid, int smem, hipStream_t stream) {
    if (hidden == 256) return gact ? launch_traj<1, true>(p, grid, smem, stream) : launch_traj<1, false>(p, grid, smem, stream);
    if (hidden == 512) return gact ? launch_traj<2, true>(p, grid, smem, stream) : launch_traj<2, false>(p, grid, smem, stream);
    return -100;
}
