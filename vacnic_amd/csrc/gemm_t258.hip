// one tile configuration of the MFMA GEMM (gemm_kernel.h) per translation unit: the 256 x 256 tile on the 8-phase counted-wait loop
// (p8_loop): <BM, BN, WM, WN, BKT, NSTAGE, PIPE, CE, DR, P8> = <256, 256, 2, 4, 64, 2, false, false, false, true>, forward layout only
#include "gemm_kernel.h"
namespace vacgemm {
int launch_t258(const GemmP& p, bool xks, bool wks, int zsplits, hipStream_t s) { return launch_gemm<256, 256, 2, 4, 64, 2, false, false, false, true>(p, xks, wks, zsplits, s); }
}  // namespace vacgemm
