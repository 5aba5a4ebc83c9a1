// select_device.h -- device read selection: the resident alignment table and the two selection kernels (rules: select_rules.h).
// Included by engine.hip.  Small non-persistent workgroups of SEL_WAVES independent waves, one window per wave, no spinning and nothing
// sized for the device: the kernels run on an engine's stream while the other engine's persistent kernels hold all but one CU's worth
// of the device, and make progress on what is left.
#pragma once
#include "select_rules.h"

struct lancet_device_reads {
  int device = 0;
  void *mem = nullptr; size_t bytes = 0;      // the one allocation
  SelTable T;                                  // device pointers into it
  const uint32_t *bases = nullptr, *good = nullptr;
  uint64_t n_base_words = 0, n_good_words = 0; // readable words (the table's + 4 / + 1)
  int32_t min_qual_trim = 0, min_qual_call = 0;
  uint64_t load_id = 0;
};

__global__ void __launch_bounds__(64 * SEL_WAVES) sel_pass1_kernel(SelTable T, const SelWin *W, int n, SelOpts O, lancet_select_summary *out) {
  __shared__ SelLds1 L[SEL_WAVES];
  const int wave = (int)(threadIdx.x >> 6), w = (int)blockIdx.x * SEL_WAVES + wave;
  if (w >= n) return;                          // (a whole wave: the waves of a workgroup never wait for each other)
  sel_pass1(T, W[w], O, &L[wave], out + w);
}
__global__ void __launch_bounds__(64 * SEL_WAVES) sel_pass2_kernel(SelTable T, const SelWin *W, const int32_t *kslice, const uint32_t *read_begin, int nk, SelOut out) {
  __shared__ SelLds2 L[SEL_WAVES];
  const int wave = (int)(threadIdx.x >> 6), k = (int)blockIdx.x * SEL_WAVES + wave;
  if (k >= nk) return;
  const uint32_t r0 = read_begin[k];
  sel_pass2(T, W[kslice[k]], r0, read_begin[k + 1] - r0, &L[wave], out);
}
