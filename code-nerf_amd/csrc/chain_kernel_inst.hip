// One chain kernel instantiation per translation unit (the Makefile compiles
// this file once per word of KERNELS with -DCN_KP/-DCN_KSB/-DCN_KTB/-DCN_KBWD/
// -DCN_KW/-DCN_KM): the unrolled chain schedules are the slowest code to
// compile, and one kernel per unit lets the build run them all in parallel.
// chain.hip only declares chain_kernel, so no other unit can instantiate one:
// the plan unit (plans.hip) references them and the link resolves them here.
#include "chain.hip"
namespace cn {
template <int P, int SB, int TB, bool BWD, int WAVES, int MODE>
__global__ CN_CHAIN_BOUNDS void chain_kernel(ChainArgs a) {
  Chain<P, SB, TB, BWD, WAVES, MODE>::run(a);
}
template __global__ void chain_kernel<CN_KP, CN_KSB, CN_KTB, CN_KBWD, CN_KW, CN_KM>(ChainArgs);
}  // namespace cn
