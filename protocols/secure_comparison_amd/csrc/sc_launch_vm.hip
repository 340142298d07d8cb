// Instances of the single-modulus interpreter k_vm and their launcher.  Compiled three times (-DSC_PART=0/1/2), each part holding a
// third of the configurations -- its rows of the list in sc_route.h -- so that the parts build in parallel and a kernel change
// recompiles only what it touches.
#include "sc_internal.h"
#include "sc_kernel_vm.h"

#ifndef SC_PART
#error "compile with -DSC_PART=0, 1 or 2"
#endif

using namespace sc;

namespace {

template <int G, int L, int WB, bool NEG1>
struct Vm {
  static constexpr uint32_t key = sc_host::launch_key(false, G, L, WB, NEG1, false, false);
  static int occupancy(sc_ctx* ctx) { return sc_host::kernel_occupancy(ctx, key, k_vm<G, L, WB, NEG1>); }
  static int launch(sc_ctx* ctx, const VmArgs& a) {
    constexpr int NG = 64 / G;
    return sc_host::launch_waves(ctx, key, k_vm<G, L, WB, NEG1>, (a.count + NG - 1) / NG, true, a, [&](uint32_t grid, VmArgs& args) {
      return sc_host::ensure_scratch(ctx, (size_t)grid * NG * a.nscratch * (G * L) * 4, &args.scratch);
    });
  }
};

#define SC_CAT_(a, b) a##b
#define SC_CAT(a, b) SC_CAT_(a, b)
#define SC_ROW(G, L, W, NEG1) {Vm<G, L, W, NEG1>::key, Vm<G, L, W, NEG1>::launch, Vm<G, L, W, NEG1>::occupancy},

}  // namespace

const sc_host::KernelRow* sc_host::SC_CAT(vm_part, SC_PART)(uint32_t key) {
  static const KernelRow rows[] = {SC_CAT(SC_VM_PART, SC_PART)(SC_ROW)};
  for (const KernelRow& row : rows)
    if (row.key == key) return &row;
  return nullptr;
}
