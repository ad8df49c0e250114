// Stand-alone host program for csrc/plan_records.h (the views plan.hip reads AabrPlanOp records through): built by
// tests/test_plan_records_host.py, also with the host sanitizers, and run directly.  Reads N x 176 bytes from the file
// named on the command line and prints, per record, `kind=K` and then `name=value` for EVERY accessor of that kind's
// view (the print list is the header's own field table): integers and pointers in decimal, floats as their 32-bit
// pattern.
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../automatic-as-built-reconstruction_amd/csrc/plan_records.h"

static void print(const char *name, int32_t v) { printf("%s=%d\n", name, v); }
static void print(const char *name, int64_t v) { printf("%s=%lld\n", name, (long long)v); }
static void print(const char *name, const void *v) { printf("%s=%llu\n", name, (unsigned long long)(uintptr_t)v); }
static void print(const char *name, float v) {
  uint32_t bits;
  memcpy(&bits, &v, 4);
  printf("%s=%u\n", name, bits);
}

#define PRINT(type, name, slot) print(#name, r.name());
#define DUMP(View, FIELDS)      \
  {                             \
    const aabr::View r{o};      \
    FIELDS(PRINT)               \
    break;                      \
  }

int main(int argc, char **argv) {
  static_assert(sizeof(AabrPlanOp) == 176, "AabrPlanOp layout is part of the C ABI");
  FILE *f = argc == 2 ? fopen(argv[1], "rb") : nullptr;
  if (!f) { printf("usage: %s FILE-OF-RECORDS\n", argv[0]); return 2; }
  std::vector<AabrPlanOp> ops;
  AabrPlanOp one;
  while (fread(&one, sizeof(one), 1, f) == 1) ops.push_back(one);
  const bool whole = feof(f) && ftell(f) == (long)(ops.size() * sizeof(one));
  fclose(f);
  if (!whole) { printf("FAILED: the file is not a whole number of records\n"); return 1; }
  for (const AabrPlanOp &o : ops) {
    printf("kind=%d\n", o.kind);
    switch (o.kind) {
    case AABR_PLAN_CONV: case AABR_PLAN_CONV_WIDE: case AABR_PLAN_CONV_WIDE_SPLIT: case AABR_PLAN_CONV_NARROW:
    case AABR_PLAN_CONV_SINGLE: DUMP(PlanConv, AABR_PLAN_CONV_FIELDS)
    case AABR_PLAN_CONV_DW: DUMP(PlanConvDw, AABR_PLAN_CONV_DW_FIELDS)
    case AABR_PLAN_BN_FWD: DUMP(PlanBnFwd, AABR_PLAN_BN_FWD_FIELDS)
    case AABR_PLAN_BN_BWD: DUMP(PlanBnBwd, AABR_PLAN_BN_BWD_FIELDS)
    case AABR_PLAN_ADD: DUMP(PlanAdd, AABR_PLAN_ADD_FIELDS)
    case AABR_PLAN_CAST: DUMP(PlanCast, AABR_PLAN_CAST_FIELDS)
    case AABR_PLAN_TAIL_JOIN: DUMP(PlanTailJoin, AABR_PLAN_TAIL_JOIN_FIELDS)
    default: printf("FAILED: unknown kind\n"); return 1;
    }
  }
  return 0;
}
