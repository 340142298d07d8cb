// Instances of the pair interpreter k_pvm and their launcher.  Compiled three times (-DSC_PART=0/1/2), see sc_launch_vm.hip.
#include "sc_internal.h"
#include "sc_kernel_pvm.h"

#ifndef SC_PART
#error "compile with -DSC_PART=0, 1 or 2"
#endif

using namespace sc;

namespace {

template <int G, int L, bool NEG1, bool STAMP, bool DIG>
struct Pvm {
  static constexpr int WB = sc_host::kPairW;
  static constexpr uint32_t key = sc_host::launch_key(true, G, L, WB, NEG1, STAMP, DIG);
  static int occupancy(sc_ctx* ctx) { return sc_host::kernel_occupancy(ctx, key, k_pvm<G, L, WB, NEG1, STAMP, DIG>); }
  static int launch(sc_ctx* ctx, const VmArgs& a) {
    constexpr int NG = 64 / G;
    // slot_per_item (segmented launches of more than one round): one wave and one table slot per group of items, so that what a
    // segment parks in the slot's table is still there for the next one; otherwise a grid-stride loop of the resident waves
    return sc_host::launch_waves(ctx, key, k_pvm<G, L, WB, NEG1, STAMP, DIG>, (a.count + NG - 1) / NG, !ctx->slot_per_item, a,
                                 [&](uint32_t grid, VmArgs& args) {
      const int rc = sc_host::ensure_scratch(ctx, (size_t)grid * NG * a.nscratch * (G * L) * 4, &args.scratch);
      if constexpr (STAMP) { if (!rc) { args.stamps = ctx->stamps; ctx->stamp_grid = grid; } }
      return rc;
    });
  }
};

#define SC_CAT_(a, b) a##b
#define SC_CAT(a, b) SC_CAT_(a, b)
#define SC_ROW(G, L, NEG1, STAMP, DIG) {Pvm<G, L, NEG1, STAMP, DIG>::key, Pvm<G, L, NEG1, STAMP, DIG>::launch, Pvm<G, L, NEG1, STAMP, DIG>::occupancy},

}  // namespace

const sc_host::KernelRow* sc_host::SC_CAT(pvm_part, SC_PART)(uint32_t key) {
  static const KernelRow rows[] = {SC_CAT(SC_PVM_PART, SC_PART)(SC_ROW)};
  for (const KernelRow& row : rows)
    if (row.key == key) return &row;
  return nullptr;
}
