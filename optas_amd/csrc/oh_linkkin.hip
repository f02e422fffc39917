// k_link_kin: batched kinematics of one link in the frame of another link -- position, rotation, quaternion, roll-pitch-yaw, geometric and
// analytical Jacobian, link axis.  Replaces RobotModel.get_link_{transform,position,rotation,quaternion,rpy,geometric_jacobian,analytical_jacobian,
// axis}_function(link, base_link, n=N) and their get_global_* forms (optas/models.py:884-1197, 1283-1409, 1517-1729).  One lane per configuration,
// streaming: 8 ndof bytes in, up to 8 (22 + 12 ndof) bytes out per unit; the definitions are at the head of oh_linkkin_unit.h.
// Templated on the length of the link chain like k_fk_jac; the base chain is walked in a run-time loop (nothing of it is kept per joint).
#include "oh_linkkin_unit.h"

#include <string>

namespace {

template <int NC>
__global__ __launch_bounds__(256) void k_link_kin(const OhLinkFrames* __restrict__ fr, const int n, const int soa, const double* __restrict__ q, const double a0,
                                                  const double a1, const double a2, const oh_link_out out) {
  link_kin_unit<NC>(fr, n, soa, q, a0, a1, a2, out);
}

}  // namespace

void oh_launch_link_kin(hipStream_t s, bool soa, const OhLinkFrames* d_frames, int n_link, int n, const double* q, const double* a3, const oh_link_out& out) {
  const dim3 b(256), g((n + 255) / 256);
  const double a0 = a3 ? a3[0] : 0.0, a1 = a3 ? a3[1] : 0.0, a2 = a3 ? a3[2] : 0.0;
  const int so = soa ? 1 : 0;
  switch (n_link) {
    case 1: hipLaunchKernelGGL((k_link_kin<1>), g, b, 0, s, d_frames, n, so, q, a0, a1, a2, out); break;
    case 2: hipLaunchKernelGGL((k_link_kin<2>), g, b, 0, s, d_frames, n, so, q, a0, a1, a2, out); break;
    case 3: hipLaunchKernelGGL((k_link_kin<3>), g, b, 0, s, d_frames, n, so, q, a0, a1, a2, out); break;
    case 4: hipLaunchKernelGGL((k_link_kin<4>), g, b, 0, s, d_frames, n, so, q, a0, a1, a2, out); break;
    case 5: hipLaunchKernelGGL((k_link_kin<5>), g, b, 0, s, d_frames, n, so, q, a0, a1, a2, out); break;
    case 6: hipLaunchKernelGGL((k_link_kin<6>), g, b, 0, s, d_frames, n, so, q, a0, a1, a2, out); break;
    case 7: hipLaunchKernelGGL((k_link_kin<7>), g, b, 0, s, d_frames, n, so, q, a0, a1, a2, out); break;
    case 8: hipLaunchKernelGGL((k_link_kin<8>), g, b, 0, s, d_frames, n, so, q, a0, a1, a2, out); break;
    default: hipLaunchKernelGGL((k_link_kin<0>), g, b, 0, s, d_frames, n, so, q, a0, a1, a2, out); break;  // 0 joints, or 9 ... OH_MAX_CHAIN
  }
}

bool oh_kernel_info_linkkin(const char* name, OhKernelInfo* out) {
  if (std::string(name) != "k_link_kin") return false;
  auto kernel = k_link_kin<7>;
  hipFuncAttributes a;
  if (hipFuncGetAttributes(&a, reinterpret_cast<const void*>(kernel)) != hipSuccess) return false;
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, 256, 0) != hipSuccess) nb = 0;
  *out = OhKernelInfo{a.numRegs, (int)a.localSizeBytes, (int)a.sharedSizeBytes, 256, nb};
  return true;
}
