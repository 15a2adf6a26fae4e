// The plan table: every (net, precision) plan the library offers, as the
// arithmetic of its forward chains and of its backward (make_chain_set).
// Adding a plan is one row here plus, for a chain kernel no other plan uses,
// one word in the Makefile's KERNELS.
#include "../../include/codenerf.h"
#include "chain_set.h"

namespace cn {
namespace {
struct PlanRow {
  int shape_blocks, texture_blocks, precision;
  ChainSet (*make)();
};
#define CN_NET_PLANS(SB, TB)                                                \
  {SB, TB, CN_FP32, make_chain_set<CN_P_FP32, CN_P_FP32, SB, TB>},          \
  {SB, TB, CN_BF16, make_chain_set<CN_P_BF16, CN_P_BF16, SB, TB>},          \
  {SB, TB, CN_BF16X3, make_chain_set<CN_P_BF16X3, CN_P_BF16X3, SB, TB>},    \
  {SB, TB, CN_BF16X3F, make_chain_set<CN_P_BF16X3, CN_P_BF16, SB, TB>}
const PlanRow kPlans[] = {CN_NET_PLANS(3, 1), CN_NET_PLANS(2, 1)};
#undef CN_NET_PLANS
}  // namespace

bool find_chain_set(int shape_blocks, int texture_blocks, int precision, ChainSet* out) {
  for (const PlanRow& r : kPlans)
    if (r.shape_blocks == shape_blocks && r.texture_blocks == texture_blocks && r.precision == precision) {
      *out = r.make();
      return true;
    }
  return false;
}

}  // namespace cn
