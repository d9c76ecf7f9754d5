// The kernel forms of an OCPSolver / ParNMPCSolver handle (idocp_amd/csrc/ocp_forms.hpp) held to their rule on the CPU, as a stand-alone
// program for the address and undefined-behaviour sanitizers (tests/test_ocp_forms_host.py builds and runs it).  The rule, as the library
// chose before the record existed and with nothing set in the environment:
//   side stream     from batch 128 on, never on a ParNMPC handle;
//   fused forward   from batch 192 on and on a chain of at most 320 nodes -- a longer chain runs S4 + K6 whatever the handle was told;
//   wide sweep      up to batch 16;
// and a mode of 0 or 1 on the record overrides the batch size.
#include <cstdio>
#include <cstdlib>

#include "ocp_forms.hpp"

using idocp_dev::OcpForms;
using idocp_dev::useFusedForward;
using idocp_dev::useSideStream;
using idocp_dev::useWideSweep;

namespace {

int failures = 0;

void expect(bool ok, const char* what, long a = -1, long b = -1) {
  if (!ok) { std::printf("FAILED: %s (%ld, %ld)\n", what, a, b); ++failures; }
}

}  // namespace

int main() {
  static_assert(idocp_dev::OcpSideStreamMinBatch == 128 && idocp_dev::OcpFusedForwardMinBatch == 192 && idocp_dev::OcpWideSweepMaxBatch == 16 &&
                idocp_dev::OcpForwardExpandMaxChain == 320, "the thresholds");
  const OcpForms def;
  expect(def.side_stream == -1 && def.fused_forward == -1 && def.riccati_wide == -1 && def.prof_dimf == 12 && def.general_axes == 0, "the default record");
  // the default record: batch, side stream, fused forward (on a chain of 320 nodes), wide sweep
  const struct { int batch; bool side, fused, wide; } table[] = {
      {1, false, false, true},     {16, false, false, true},   {17, false, false, false}, {127, false, false, false},
      {128, true, false, false},   {191, true, false, false},  {192, true, true, false},  {1024, true, true, false}};
  for (const auto& row : table) {
    expect(useSideStream(def, row.batch, false) == row.side, "side stream by batch size", row.batch);
    expect(!useSideStream(def, row.batch, true), "ParNMPC: never a side stream", row.batch);
    expect(useFusedForward(def, row.batch, 320) == row.fused, "fused forward by batch size, 320 nodes", row.batch);
    expect(useFusedForward(def, row.batch, 32) == row.fused, "fused forward by batch size, 32 nodes", row.batch);
    expect(!useFusedForward(def, row.batch, 321), "321 nodes: S4 + K6", row.batch);
    expect(useWideSweep(def, row.batch) == row.wide, "wide sweep by batch size", row.batch);
    std::printf("forms %d: side %d fused %d wide %d\n", row.batch, (int)useSideStream(def, row.batch, false), (int)useFusedForward(def, row.batch, 320),
                (int)useWideSweep(def, row.batch));
  }
  // every forced mode, at every batch size of the table
  for (const auto& row : table)
    for (int mode = 0; mode <= 1; ++mode) {
      OcpForms f;
      f.side_stream = mode;
      expect(useSideStream(f, row.batch, false) == (mode == 1), "side stream forced", row.batch, mode);
      expect(!useSideStream(f, row.batch, true), "ParNMPC: never a side stream, forced or not", row.batch, mode);
      expect(useFusedForward(f, row.batch, 320) == row.fused && useWideSweep(f, row.batch) == row.wide, "forcing the side stream moves nothing else", row.batch, mode);
      f = OcpForms();
      f.fused_forward = mode;
      expect(useFusedForward(f, row.batch, 320) == (mode == 1), "fused forward forced, 320 nodes", row.batch, mode);
      expect(!useFusedForward(f, row.batch, 321), "fused forward forced, 321 nodes: S4 + K6", row.batch, mode);
      expect(useSideStream(f, row.batch, false) == row.side && useWideSweep(f, row.batch) == row.wide, "forcing the forward sweep moves nothing else", row.batch, mode);
      f = OcpForms();
      f.riccati_wide = mode;
      expect(useWideSweep(f, row.batch) == (mode == 1), "wide sweep forced", row.batch, mode);
      expect(useSideStream(f, row.batch, false) == row.side && useFusedForward(f, row.batch, 320) == row.fused, "forcing the backward sweep moves nothing else", row.batch, mode);
    }
  if (failures) { std::printf("ocp forms: %d failures\n", failures); return EXIT_FAILURE; }
  std::printf("ocp forms: ok\n");
  return EXIT_SUCCESS;
}
