// The per-triple statements of the body-against-body overlap test (DESIGN.md "Body against body"), shared by csrc/body_overlap.hip and by
// the host rehearsal tools/body_overlap_host_check.hip.  Everything that decides membership (box, threshold) is a comparison; the winding
// number is fp32 within a chunk of BO_CHUNK faces and fp64 across the chunks of a slice of BO_SLICE faces and across the slices.  The box
// tests (geom_in_box, geom_boxes_meet), the fp32 normal (geom_normal) and the solid angle (geom_half_omega) are csrc/geom_shared.h.
#pragma once
#include "geom_shared.h"
#include <stdint.h>

// The handle of psi_body_overlap_create, which csrc/body_depth.hip takes as well: the one topology of every body, on the device
struct psi_body_overlap {
    char *blob;                // the one allocation (csrc/blob.h)
    int32_t *d_faces;          // [F,3]
    int V, F;
};

constexpr int BO_CHUNK = 256;       // consecutive faces summed in fp32: a constant of the contract, not a launch parameter
constexpr int BO_SLICE = 2048;      // consecutive faces whose chunk sums are added in fp64, in order, before the slices are
constexpr int BO_CHUNKS_PER_SLICE = BO_SLICE / BO_CHUNK;

GEOM_FN float bo_w_of_sum(double s) { return (float)(s / 6.283185307179586476925286766559); }

GEOM_FN bool bo_inside(float w) { return w > 0.5f; }

GEOM_FN int bo_slices(int F) { return (F + BO_SLICE - 1) / BO_SLICE; }
