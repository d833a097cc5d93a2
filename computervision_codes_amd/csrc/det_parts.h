// Host side of the deterministic (`_det`) forms of the training reductions: the parts a launch stores into its workspace.
// The rule: an op has ONE function from its shape to a DetParts (and, where the launch needs them, its slab / split numbers).  The host-only plan
// query (`mt4_*_det_plan`), the workspace check of the deterministic entry and the grids of both launch forms read that one value, so a workspace
// the plan calls large enough is the one the launch accepts.
#pragma once
#include "mt4_common.h"

struct DetParts {
    int32_t form;         // the launch form the op's plan documents (0 where there is one)
    int32_t nparts;       // parts = the workgroups along the reduced dimension (gridDim.y / .z, or the row-split count), of both launch forms
    int64_t part_elems;   // elements of a part = its stride in the workspace
    int32_t esize;        // bytes of an element
    int64_t bytes() const { return (int64_t)nparts * part_elems * esize; }
};

// the tail every plan query shares: the four optional out-parameters
static inline int det_plan_out(const DetParts& p, int32_t* form, int32_t* nparts, int64_t* part_elems, int64_t* ws_bytes) {
    if (form) *form = p.form;
    if (nparts) *nparts = p.nparts;
    if (part_elems) *part_elems = p.part_elems;
    if (ws_bytes) *ws_bytes = p.bytes();
    return MT4_OK;
}

// train-mode BatchNorm reductions (statistics and backward, both tensor types): parts [slabs][2][C] float64, one per row slab of the 1024-thread reduction
static inline DetParts bn_parts(long long M, int C) { return {0, bn_reduce_slabs(M, C), 2LL * C, (int32_t)sizeof(double)}; }
