// Private: entry points shared between gemm.hip (dispatcher) and gemm_big.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "common.h"
#include "g2vlm_hip.h"

bool g2v_gemm_big_eligible(const g2v_gemm_desc* d);
int g2v_gemm_big_height(const g2v_gemm_desc* d);
int g2v_gemm_big_launch(const g2v_gemm_desc* d, hipStream_t s);
bool g2v_gemm_8p_supported(const g2v_gemm_desc* d);
bool g2v_gemm_8p_preferred(const g2v_gemm_desc* d);
int g2v_gemm_8p_height(const g2v_gemm_desc* d);
bool g2v_gemm_8p_four_waves(const g2v_gemm_desc* d);
int g2v_gemm_8p_launch(const g2v_gemm_desc* d, hipStream_t s);
// gemm_4w.hip: the four-wave form of the same tile, launched by g2v_gemm_8p_launch with the arguments it packed (gemm_tile256.h)
struct T256Args;
int g2v_gemm_4w_launch(const T256Args& a, int epilogue, int bm, hipStream_t s);
bool g2v_gemm_skinny_eligible(const g2v_gemm_desc* d);
void g2v_gemm_skinny_split(const g2v_gemm_desc* d, int M, int* S, int* KS);
int g2v_gemm_skinny_launch(const g2v_gemm_desc* d, hipStream_t s);

// f(std::integral_constant<int, EPI>{}) for the epilogue of a launch: the switch from the run-time value to the template argument
template <class F>
int g2v_gemm_with_epilogue(int epilogue, F&& f) {
  switch (epilogue) {
    case G2V_EPI_BF16: return f(std::integral_constant<int, G2V_EPI_BF16>{});
    case G2V_EPI_GELU: return f(std::integral_constant<int, G2V_EPI_GELU>{});
    case G2V_EPI_QUICKGELU: return f(std::integral_constant<int, G2V_EPI_QUICKGELU>{});
    case G2V_EPI_SWIGLU: return f(std::integral_constant<int, G2V_EPI_SWIGLU>{});
    case G2V_EPI_RES_F32: return f(std::integral_constant<int, G2V_EPI_RES_F32>{});
    case G2V_EPI_RES_BF16: return f(std::integral_constant<int, G2V_EPI_RES_BF16>{});
    default: return G2V_ERR_ARG;
  }
}
