// Device arithmetic of the PCA step shared by the BoF kernels (bow.hip) and the vocabulary trainer (trainbow.hip), so
// that training rows and query vectors are projected by the same chain of float operations.
#pragma once

#include <hip/hip_runtime.h>

namespace sfmloc {

// PcaWrapper::calcPcaProject (PcaWrapper.cpp:67-89) for one component: project, then divide by the eigenvalue.
// float32, in input-dimension order, unfused (-ffp-contract=off), so the oracle's sequential loop gives the same bits.
__device__ __forceinline__ float bof_pca_component(const float *x, const float *mean, const float *evec_row, int in_dim,
                                                   float eval) {
  float acc = 0.0f;
  for (int i = 0; i < in_dim; ++i) {
    const float c = x[i] - mean[i];
    const float pr = c * evec_row[i];
    acc = acc + pr;
  }
  return acc / eval;
}

}  // namespace sfmloc
