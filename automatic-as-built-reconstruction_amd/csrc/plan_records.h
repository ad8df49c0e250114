// plan_records.h -- which slot of an AabrPlanOp record (include/aabr_hip.h) holds which operand, per record layout:
// the C++ side of sparseconvnet/plan_records.py.  Host-only and free of HIP calls, like plan_tail.h and the *_tiles.h
// decision headers: tests/plan_records_host_harness.cpp compiles it alone and prints every field of records the Python
// side wrote (tests/test_plan_records_host.py).
//
// One table per layout: X(type, name, slot) for every slot the layout uses, the names of the Python table.  A view is a
// `const AabrPlanOp &` with one inline accessor per line of its table; plan.hip reads records through views only.  A
// new slot goes into BOTH tables and into the header's prose; the host test fails when the two tables disagree.
//
// Pointer operands come back as `const void *` (only read by every entry point the record reaches) or `void *`; the
// storage flag of the record decides what they point to.  Two names on one slot are the overlaps the Python table
// declares: which name applies follows from the record's kind.
#pragma once
#include <stdint.h>
#include "../../include/aabr_hip.h"

// AABR_PLAN_CONV, _CONV_WIDE, _CONV_WIDE_SPLIT, _CONV_NARROW, _CONV_SINGLE
#define AABR_PLAN_CONV_FIELDS(X)                                                                                      \
  X(int32_t, n_in, i32[0]) X(int32_t, n_out, i32[1]) X(int32_t, vol, i32[2]) X(int32_t, conv_flags, i32[3])          \
  X(int32_t, tile_rows, i32[4]) X(int32_t, bwd_stats, i32[5]) X(float, leak, f32[0])                                 \
  X(int64_t, rows_in, i64[0]) X(int64_t, V_out, i64[1])                                                              \
  X(const void *, in, p[0]) X(void *, out, p[1]) X(const void *, gather, p[2]) X(const void *, residual, p[3])       \
  X(const void *, bias, p[4]) X(void *, wpack, p[5]) X(void *, stats, p[6]) X(const void *, bn_in, p[7])             \
  X(const void *, save_mean, p[8]) X(const void *, save_invstd, p[9]) X(const void *, bn_weight, p[10])              \
  X(const void *, bn_bias, p[11])                                                                                    \
  /* overlaps: CONV / CONV_NARROW p3; CONV_WIDE_SPLIT i32[5], p6; bf16 backward statistics p9 */                      \
  X(const void *, weight, p[3]) X(int32_t, parts, i32[5]) X(void *, scratch, p[6]) X(const void *, bn_out, p[9])

#define AABR_PLAN_CONV_DW_FIELDS(X)                                                                                   \
  X(int32_t, n_in, i32[0]) X(int32_t, n_out, i32[1]) X(int32_t, vol, i32[2])                                         \
  X(int64_t, V_out, i64[0]) X(int64_t, max_chunks, i64[1])                                                           \
  X(const void *, in, p[0]) X(const void *, d_out, p[1]) X(const void *, pairs, p[2]) X(void *, dW, p[3])            \
  X(void *, d_bias, p[4]) X(void *, scratch, p[5])

#define AABR_PLAN_BN_FWD_FIELDS(X)                                                                                    \
  X(int32_t, planes, i32[0]) X(int32_t, train, i32[1]) X(int32_t, nparts, i32[2])                                    \
  X(float, eps, f32[0]) X(float, momentum, f32[1]) X(float, leak, f32[2]) X(int64_t, rows, i64[0])                   \
  X(const void *, in, p[0]) X(void *, out, p[1]) X(void *, save_mean, p[2]) X(void *, save_invstd, p[3])             \
  X(void *, running_mean, p[4]) X(void *, running_var, p[5]) X(const void *, weight, p[6]) X(const void *, bias, p[7]) \
  X(void *, scratch, p[8]) X(const double *, parts, p[9])

// `parts`: the address of the partial sums travels in i64[1]
#define AABR_PLAN_BN_BWD_FIELDS(X)                                                                                    \
  X(int32_t, planes, i32[0]) X(int32_t, nparts, i32[1]) X(float, leak, f32[2])                                       \
  X(int64_t, rows, i64[0]) X(const double *, parts, i64[1])                                                          \
  X(const void *, in, p[0]) X(void *, d_in, p[1]) X(const void *, out, p[2]) X(const void *, d_out, p[3])            \
  X(const void *, save_mean, p[4]) X(const void *, save_invstd, p[5]) X(const void *, weight, p[6])                  \
  X(void *, d_weight, p[7]) X(void *, d_bias, p[8]) X(void *, scratch, p[9]) X(const void *, bias, p[10])            \
  X(const void *, d_in_add, p[11])

#define AABR_PLAN_ADD_FIELDS(X) X(int64_t, n, i64[0]) X(const void *, a, p[0]) X(const void *, b, p[1]) X(void *, out, p[2])
#define AABR_PLAN_CAST_FIELDS(X) X(int64_t, n, i64[0]) X(const void *, in, p[0]) X(void *, out, p[1])
#define AABR_PLAN_TAIL_JOIN_FIELDS(X) X(int64_t, ticket, i64[0])

namespace aabr {

#define AABR_PLAN_ACCESSOR(type, name, slot) \
  type name() const { return (type)o.slot; }
#define AABR_PLAN_VIEW(View, FIELDS) \
  struct View {                      \
    const AabrPlanOp &o;             \
    FIELDS(AABR_PLAN_ACCESSOR)       \
  }
AABR_PLAN_VIEW(PlanConv, AABR_PLAN_CONV_FIELDS);
AABR_PLAN_VIEW(PlanConvDw, AABR_PLAN_CONV_DW_FIELDS);
AABR_PLAN_VIEW(PlanBnFwd, AABR_PLAN_BN_FWD_FIELDS);
AABR_PLAN_VIEW(PlanBnBwd, AABR_PLAN_BN_BWD_FIELDS);
AABR_PLAN_VIEW(PlanAdd, AABR_PLAN_ADD_FIELDS);
AABR_PLAN_VIEW(PlanCast, AABR_PLAN_CAST_FIELDS);
AABR_PLAN_VIEW(PlanTailJoin, AABR_PLAN_TAIL_JOIN_FIELDS);
#undef AABR_PLAN_VIEW
#undef AABR_PLAN_ACCESSOR

} // namespace aabr
