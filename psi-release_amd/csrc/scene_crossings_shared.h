// What csrc/scene_crossings.hip shares with its host rehearsal tools/scene_crossings_host_check.hip: the sort key
// of a pair (body i, body face s, scene triangle t) and the host half of psi_scene_crossings_create, which is plain C++ without a HIP
// call: the records of the chunk order, the chunk boxes and the scene's box.  The per-pair statements (sc_pair, sc_face_box) and the
// Morton order of the triangles (sc_morton_order) are csrc/surface_crossings_shared.h, the closed-box test csrc/geom_shared.h.
#pragma once
#include "surface_crossings_shared.h"
#include <string.h>

constexpr int SCN_REC_ROWS = 3;         // float4 rows of a record: q0.xyz q1.x | q1.yz q2.xy | q2.z caller's index 0 0

// The sort key of a pair: ascending keys are ascending (i, s, t).  The caller guarantees B * F * nf < 2^63.
SC_FN long long scn_key(int i, int s, int t, int F, int nf) { return ((long long)i * F + s) * nf + t; }

SC_FN void scn_unkey(long long key, int F, int nf, int out[3])
{
    out[2] = (int)(key % nf);
    key /= nf;
    out[1] = (int)(key % F);
    out[0] = (int)(key / F);
}

// B * F * nf < 2^63, decided in integers
static inline bool scn_key_fits(long long B, long long F, long long nf)
{
    const long long top = 0x7fffffffffffffffll;
    return B >= 1 && F >= 1 && nf >= 1 && B <= top / F && B * F <= top / nf;
}

struct ScnBuilt {
    std::vector<int32_t> order;         // [nf] the caller's triangle at every position of the chunk order
    std::vector<float> recs;            // [nf, SCN_REC_ROWS * 4]
    std::vector<float> chunk_boxes;     // [n_chunks, 6] min xyz, max xyz
    float box[6];                       // of the whole scene
};

enum { SCN_OK = 0, SCN_NO_FACES = 1, SCN_BAD_INDEX = 2, SCN_NOT_FINITE = 3 };

// The host half of create.  The triangles in Morton order (sc_morton_order); chunks of SC_CHUNK positions; boxes by comparisons only.
// *bad: the first offending triangle.
static inline int scn_build(const float *v, int nv, const int32_t *f, long long nf, ScnBuilt *o, long long *bad)
{
    *bad = -1;
    if (nf < 1 || nf > 0x7fffffffll) return SCN_NO_FACES;
    for (long long t = 0; t < nf; t++)
        for (int k = 0; k < 3; k++) {
            const int32_t id = f[t * 3 + k];
            if (id < 0 || id >= nv) { *bad = t; return SCN_BAD_INDEX; }
            for (int a = 0; a < 3; a++)
                if (!std::isfinite(v[(size_t)id * 3 + a])) { *bad = t; return SCN_NOT_FINITE; }
        }
    o->order.resize((size_t)nf);
    sc_morton_order(v, f, nf, o->order.data());             // (every referenced coordinate is finite: so are the sums of three in fp64)
    const long long nK = (nf + SC_CHUNK - 1) / SC_CHUNK;
    o->recs.assign((size_t)nf * SCN_REC_ROWS * 4, 0.0f);
    o->chunk_boxes.resize((size_t)nK * 6);
    for (int a = 0; a < 3; a++) o->box[a] = INFINITY, o->box[3 + a] = -INFINITY;
    for (long long k = 0; k < nK; k++) {
        float clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (long long pos = k * SC_CHUNK; pos < std::min(nf, (k + 1) * SC_CHUNK); pos++) {
            const int32_t t = o->order[(size_t)pos];
            float q[3][3], flo[3], fhi[3], *r = &o->recs[(size_t)pos * SCN_REC_ROWS * 4];
            for (int j = 0; j < 3; j++)
                for (int a = 0; a < 3; a++) q[j][a] = r[j * 3 + a] = v[(size_t)f[(size_t)t * 3 + j] * 3 + a];
            memcpy(r + 9, &t, sizeof(t));
            sc_face_box(q, flo, fhi);
            for (int a = 0; a < 3; a++) clo[a] = fminf(clo[a], flo[a]), chi[a] = fmaxf(chi[a], fhi[a]);
        }
        for (int a = 0; a < 3; a++) {
            o->chunk_boxes[(size_t)k * 6 + a] = clo[a];
            o->chunk_boxes[(size_t)k * 6 + 3 + a] = chi[a];
            o->box[a] = fminf(o->box[a], clo[a]);
            o->box[3 + a] = fmaxf(o->box[3 + a], chi[a]);
        }
    }
    return SCN_OK;
}
