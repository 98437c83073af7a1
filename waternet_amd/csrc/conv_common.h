// Shared by conv_fwd.hip and conv_wgrad.hip: the fragment K-mapping switch,
// the host-side helpers every tier's launch goes through, the counted waits
// and the glds patch-image slot map of the patch kernels of both units.
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

// Counted waits: the count is an "n" operand, so one template serves every
// ring depth instead of a ladder of literal asm strings.
template <int N>
WN_DEVFN void wait_vmcnt() {
  static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit field");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
template <int N>
WN_DEVFN void wait_lgkmcnt() {
  static_assert(N >= 0 && N <= 15, "lgkmcnt is a 4-bit field");
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
}

// ---------------------------------------------------------------------------
// Patch image: plain [pixel][COLS] bf16 rows of COLS/8 16 B channel chunks,
// filled by global_load_lds. glds writes lane-linearly (slot s lands at byte
// 16*s), so a bank swizzle cannot move the destination; it XORs the chunk
// INDEX inside a pixel row instead, which moves whole 16 B chunks, and each
// slot sources the chunk that belongs where it lands. Swz::chunk_xor(pix,
// COLS) is the XOR of a pixel row; it is a policy of the READ instruction the
// image serves, and each kernel proves its own reads conflict-free on off().
// ---------------------------------------------------------------------------
template <class Swz>
struct PatchImage {
  // byte offset of 16 B channel chunk `chunk` of pixel row `pix`
  static constexpr int off(int pix, int chunk, int COLS) {
    return pix * COLS * 2 + ((chunk ^ Swz::chunk_xor(pix, COLS)) << 4);
  }
  // glds staging slot -> image pixel row / SOURCE 16 B channel chunk
  static constexpr int slot_pix(int slot, int COLS) {
    return slot / (COLS / 8);
  }
  static constexpr int slot_chunk(int slot, int COLS) {
    return (slot % (COLS / 8)) ^ Swz::chunk_xor(slot_pix(slot, COLS), COLS);
  }
  // the slot map lands slot s at byte 16*s and covers every chunk of every
  // pixel row exactly once (lane-linear glds image)
  static constexpr bool linear(int NPIX, int COLS) {
    const int CPR = COLS / 8;
    for (int pix = 0; pix < NPIX; ++pix) {
      unsigned seen = 0;
      for (int c = 0; c < CPR; ++c) {
        const int s = pix * CPR + c;
        if (slot_pix(s, COLS) != pix) return false;
        const int ch = slot_chunk(s, COLS);
        if (ch < 0 || ch >= CPR) return false;
        if (off(pix, ch, COLS) != 16 * s) return false;
        seen |= 1u << ch;
      }
      if (seen != (1u << CPR) - 1) return false;
    }
    return true;
  }
};
