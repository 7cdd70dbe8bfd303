// The stand-in launchers of tests/host_stub_launchers.cpp with ONE difference: launch_tim_graph_mfma records the
// `phase` argument of every call (tests/test_host_graph_routes.py: which store mode K1 and the fix-up were given, where
// the closure's pair phase, the mirror and the rebuilds were enqueued).  The fixed file is compiled into this one with
// its own launcher under another name.
#include <vector>

#define launch_tim_graph_mfma launch_tim_graph_mfma_unrecorded
#include "host_stub_launchers.cpp"
#undef launch_tim_graph_mfma

std::vector<int> g_route_phases;  // (one host thread: the driver uses the synchronous API only)

namespace thip {

void launch_tim_graph_mfma(hipStream_t, int phase, const ProbDesc*, int, int, int64_t, const double*, const double*, void*, void*,
                           void*, int64_t, uint64_t*, ProbState*, int32_t*, double, double) {
  ++g_stub_launches;
  g_route_phases.push_back(phase);
}

}  // namespace thip
