// TEST INFRASTRUCTURE ONLY: the launch coordinates of the sequential HIP stand-in (tests/emul/hip/hip_runtime.h) for the host build of
// jodo_amd/csrc/train_step.hip.
#include <hip/hip_runtime.h>
thread_local emu_idx threadIdx, blockIdx;
thread_local dim3 blockDim, gridDim;
