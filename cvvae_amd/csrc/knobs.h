// knobs.h -- the environment knobs of the library as ONE table behind ONE accessor.  Plain C++ (no HIP types).
//
// The knobs are tuning, A/B and debug aids: they decide which kernel runs, and so which bits come out.  The table holds the weight
// gradient's knobs (wgrad_kernel.hip reads the environment nowhere else: tests/test_knobs.py); the forward convolution's knobs
// (CVVAE_CONV_*, tools/README.md) are still read where they are used, in cvvae_api.hip and conv_kernel.h, and are to move here.
//
// A row is  X(id, "NAME", rule, default, read, "purpose"):
//   rule   how the variable's text becomes the value when the variable is SET (unset: the default)
//            INT      atoi(text)
//            REAL     atof(text)
//            NONZERO  atoi(text) != 0        -- "NAME=0 switches it off" for a default of 1, "NAME=1 switches it on" for 0
//                                               (text that is no number counts as 0)
//            PRESENT  1 whatever the text    -- set means on
//            TEXT     the text itself (default: null)
//   read   ONCE      parsed at the first use in the process and kept: a launch never calls getenv for these.  Setting one after the
//                    first launch changes NOTHING -- a test of such a knob needs a child process.
//          PER_CALL  parsed at every use: the GPU tests flip these inside one process.
// knob<KNOB_id>() enforces the read policy; knob_int / knob_real / knob_on / knob_text also check the rule at compile time.
#pragma once
#include <stdlib.h>

namespace cvvae {

#define CVVAE_KNOBS(X)                                                                                                         \
  X(WGRAD_DMA, "CVVAE_WGRAD_DMA", NONZERO, 1, ONCE, "0: the register-staged weight-gradient kernel for every layer")           \
  X(WGRAD_WGS, "CVVAE_WGRAD_WGS", INT, 0, ONCE, "> 0: target number of weight-gradient workgroups instead of the rounds rule") \
  X(WGRAD_FAST, "CVVAE_WGRAD_FAST", NONZERO, 1, PER_CALL, "0: per-lane 64-bit wave-load addresses in wgrad_dma_kernel")

enum KnobRule { KNOB_INT, KNOB_REAL, KNOB_NONZERO, KNOB_PRESENT, KNOB_TEXT };
enum KnobRead { KNOB_ONCE, KNOB_PER_CALL };

enum Knob {
#define CVVAE_KNOB_ID(id, name, rule, def, read, purpose) KNOB_##id,
  CVVAE_KNOBS(CVVAE_KNOB_ID)
#undef CVVAE_KNOB_ID
  KNOB_COUNT
};

struct KnobRow {
  const char* name;
  KnobRule rule;
  double def;
  KnobRead read;
  const char* purpose;
};

inline constexpr KnobRow kKnobs[KNOB_COUNT] = {
#define CVVAE_KNOB_ROW(id, name, rule, def, read, purpose) {name, KNOB_##rule, def, KNOB_##read, purpose},
    CVVAE_KNOBS(CVVAE_KNOB_ROW)
#undef CVVAE_KNOB_ROW
};

struct KnobValue {
  double num;        // INT / REAL / NONZERO / PRESENT (every int is exact in a double)
  const char* text;  // TEXT: the variable's text, or null
};

inline KnobValue knob_parse(const KnobRow& r) {
  const char* s = getenv(r.name);
  if (!s) return {r.def, nullptr};
  switch (r.rule) {
    case KNOB_INT: return {(double)atoi(s), s};
    case KNOB_REAL: return {atof(s), s};
    case KNOB_NONZERO: return {atoi(s) != 0 ? 1.0 : 0.0, s};
    case KNOB_PRESENT: return {1.0, s};
    default: return {0.0, s};
  }
}

template <Knob K>
inline KnobValue knob() {
  if constexpr (kKnobs[K].read == KNOB_ONCE) {
    static const KnobValue v = knob_parse(kKnobs[K]);
    return v;
  } else {
    return knob_parse(kKnobs[K]);
  }
}

template <Knob K>
inline int knob_int() {
  static_assert(kKnobs[K].rule == KNOB_INT, "not an INT knob");
  return (int)knob<K>().num;
}
template <Knob K>
inline double knob_real() {
  static_assert(kKnobs[K].rule == KNOB_REAL, "not a REAL knob");
  return knob<K>().num;
}
template <Knob K>
inline bool knob_on() {
  static_assert(kKnobs[K].rule == KNOB_NONZERO || kKnobs[K].rule == KNOB_PRESENT, "not an on / off knob");
  return knob<K>().num != 0.0;
}
template <Knob K>
inline const char* knob_text() {
  static_assert(kKnobs[K].rule == KNOB_TEXT, "not a TEXT knob");
  return knob<K>().text;
}

}  // namespace cvvae
