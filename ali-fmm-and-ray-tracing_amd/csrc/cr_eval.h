// cr_eval.h — one evaluation of a cr_math.h function through the operators' macros (AF_ATAN ... of
// device_common.h), shared by the two kernels behind alifmm_cr_math: utils.hip's reads the tables
// from the global constants, cr_eval.hip's (CR_LDS_TABLES) from LDS.
#pragma once
#include "device_common.h"

namespace af {

constexpr int kCrEvalThreads = 256;

// fn 0 atan, 1 sin, 2 cos, 3 tan -> *o; 4 sincos -> sin *o, cos *o2 (the host checked fn and o2)
AF_DEV void cr_eval_one(int fn, double x, double* o, double* o2) {
  switch (fn) {
    case 0: *o = AF_ATAN(x); break;
    case 1: *o = AF_SIN(x); break;
    case 2: *o = AF_COS(x); break;
    case 3: *o = AF_TAN(x); break;
    default: {
      double s, c;
      AF_SINCOS(x, &s, &c);
      *o = s;
      *o2 = c;
    }
  }
}

// blocks of kCrEvalThreads for n arguments; 0: n does not fit a grid
static inline unsigned cr_eval_blocks(long long n) {
  const long long b = (n + kCrEvalThreads - 1) / kCrEvalThreads;
  return b > 0x7fffffffLL ? 0u : (unsigned)b;
}

}  // namespace af
