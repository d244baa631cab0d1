// the 256x256 ping-pong configuration with the ARGMAX variant of the fused LM-head cross-entropy forward epilogue (out_mode 3):
// a kernel of its own, launched only by vacnic_lmhead_eval — the kernels of gemm_t256ce.hip and gemm_t256cels.hip are untouched by it
#include "gemm_kernel.h"
namespace vacgemm {
int launch_t256ceam(const GemmP& p, bool xks, bool wks, int zsplits, hipStream_t s) { return launch_gemm_ce_argmax<256, 256, 2, 4, 32, 4, true>(p, xks, wks, zsplits, s); }
}  // namespace vacgemm
