// Shared by conv_fwd.hip and conv_wgrad.hip: the fragment K-mapping switch
// and the host-side helpers every tier's launch goes through.
//
// Design notes (MI355X), common to all conv kernels:
//   - Cp (physical channels) is a power of two >= 16; pad channels are
//     zero by construction everywhere, so no channel masking in the GEMM.
//   - out-of-range staging lanes (conv halo, channel pad, M tail) source a
//     16 B zero buffer instead of skipping their DMA (zero16_for below).
//
// WN_MFMA_KMAP: fragment K mapping, measured by probe_mfma.hip — 0 on this
// hardware (lane group g consumes reduction elements k = g*8+e).
#pragma once

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cmath>
#include <type_traits>

#include "common.h"

#ifndef WN_MFMA_KMAP
#define WN_MFMA_KMAP 0
#endif

inline int log2i(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  TORCH_CHECK((1 << l) == v, "value not a power of two: ", v);
  return l;
}

// Runtime int -> template constant: calls f(std::integral_constant<int, V>)
// for the V in Vs... equal to `value`, and raises naming `what` (the knob or
// argument) for a value outside the list.
template <int... Vs, class F>
inline void dispatch_int(int value, const char* what, F&& f) {
  const bool hit =
      ((value == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) ||
       ...);
  TORCH_CHECK(hit, "unsupported ", what, " ", value);
}

// As dispatch_int, but a value outside the list runs the Default arm (which
// must be in the list) instead of raising.
template <int Default, int... Vs, class F>
inline void dispatch_int_or(int value, F&& f) {
  static_assert(((Default == Vs) || ...), "default not in the list");
  const bool listed = ((value == Vs) || ...);
  dispatch_int<Vs...>(listed ? value : Default, "value", f);
}

// 16 B of zeros on `like`'s device: the glds source of halo / pad / tail
// lanes. Cached per host thread, re-created when the device changes.
inline const bf16_t* zero16_for(const at::Tensor& like) {
  static thread_local at::Tensor zero16;
  if (!zero16.defined() || zero16.device() != like.device())
    zero16 = at::zeros({8}, like.options());
  return (const bf16_t*)zero16.data_ptr();
}
