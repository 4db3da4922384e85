// host_seq.h — what the two host-only sequencing files (layers.hip, model.hip) share: the early return on a failed call and the
// byte size of a storage type.
#pragma once
#include "gt_common.h"

#define GT_TRY(call)                \
  do {                              \
    int rc__ = (call);              \
    if (rc__ != GT_OK) return rc__; \
  } while (0)

static inline size_t gt_elt_bytes(int dtype) { return dtype == GT_BF16 ? 2 : 4; }
