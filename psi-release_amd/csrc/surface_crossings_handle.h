// The psi_surface_crossings handle, shared by csrc/surface_crossings.hip (which makes and frees it), csrc/scene_crossings.hip (whose bodies
// come with it) and csrc/crossing_field.hip (which reads the faces of the pairs it is given, in the caller's face indices).
#pragma once
#include <stdint.h>

struct psi_surface_crossings {
    char *blob;                // the one allocation behind the five buffers (csrc/blob.h): d_faces | d_orig | d_part | d_skip | d_caller
    int32_t *d_faces;          // [F,3] in chunk order
    int32_t *d_orig;           // [F] the caller's index of the face at a position
    int32_t *d_part;           // [F] in chunk order, or null
    uint8_t *d_skip;           // [P,P], or null
    int V, F, P;
    int32_t *d_caller;         // [F,3] in the caller's order: the face of a reported index
};
