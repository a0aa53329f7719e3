// Do two operator views share memory? (views_overlap.hip: host arithmetic on two wg_view_shape and two byte addresses -- no kernel, no device call, no context,
// nothing else of the library.) The operator front-end (api.hip) asks it for every (written, read) pair of a call and refuses the call with WG_ERR_ALIASED when the
// answer is yes; tests read it through wg_debug_views_overlap, and tests/cpp/overlap_check.cpp links the unit alone under the host sanitizers.
#pragma once
#include <cstdint>

#include "../../include/wgebra_hip.h"

// The footprint of a view: the bytes [base + e * elem_size, + elem_size) of every element e = t * stride_mat + offset + i + j * stride it addresses
// (i < size[0], j < size[1], t < size[2]); `base` is the byte address of element 0 of the buffer the view indexes. A view with a zero size has no footprint.
// Returns 1 when the two footprints share a byte, 0 when they do not. Decided in three steps:
//   1. the byte intervals [first byte, last byte] of the two views: disjoint intervals are disjoint footprints (the common case: a few integer comparisons);
//   2. each view as column runs -- one contiguous run per (column, matrix); columns at most `rows` apart and matrices at most one matrix apart are folded into one run
//      first, so a dense matrix or cube is ONE run --: while the two views have at most WG_VIEWS_OVERLAP_MAX_RUNS runs between them the runs are walked in address
//      order and the answer is exact (*exact = 1);
//   3. above that bound the answer is 1 ("overlaps") whatever the truth, and *exact = 0.
// `exact` may be NULL. Never answers 0 for footprints that intersect.
int wg_views_overlap(const wg_view_shape &a, uint64_t byte_base_a, const wg_view_shape &b, uint64_t byte_base_b, uint32_t elem_size, int *exact);
