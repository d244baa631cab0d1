// the 256x256 ping-pong configuration with the LABEL-SMOOTHING variants of the fused LM-head cross-entropy epilogues (out_mode 3 / 4):
// a kernel of its own, launched only with label_smoothing > 0 — the kernels of gemm_t256ce.hip are untouched by the option
#include "gemm_kernel.h"
namespace vacgemm {
int launch_t256cels(const GemmP& p, bool xks, bool wks, int zsplits, hipStream_t s) { return launch_gemm_ce_smooth<256, 256, 2, 4, 32, 4, true>(p, xks, wks, zsplits, s); }
}  // namespace vacgemm
