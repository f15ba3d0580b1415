// The statements of the conic distance field of a triangle, shared by csrc/crossing_field.hip and by the host
// rehearsal tools/crossing_field_host_check.hip: the receiver record, the evaluation of a point in it, and the reverse mode of both.  No
// contraction; division and square root are IEEE-rounded on the device as on the host, and the only operations are + - * / sqrt and
// comparisons, so the fp32 NumPy restatement (tests/crossing_field_ref.py) mirrors this file line for line and gives the same bits.
//
//   record      of the receiver (a, b, c):  e1 = b - a, e2 = c - a, N = e1 x e2, N2 = N.N, len = sqrt(N2), n = N / len,
//               m = (e1.e1) (e2 x N) + (e2.e2) (N x e1), den = 2 N2, q = m / den (the circumcentre minus a), o = a + q, r = sqrt(q.q)
//   evaluation  of p:  w = p - o, h = n.w, t = w - h n, rho = sqrt(t.t);  gate 1: h < sigma;  D = r (1 - h / sigma), Phi = rho / D;
//               gate 2: Phi < 1;  Y = (1 - h) - sigma for h <= -sigma, else (c0 - c1 h) - (c2 h) h;  Psi = (1 - Phi) Y
//   constants   s2 = 2 sigma, c2 = (1 - s2) / (s2 s2), c1 = 1 / s2, c0 = (3 - s2) / 4
// A cross component is a*b - c*d, a dot product (x + y) + z.  Both gates are positive comparisons: a NaN or an infinity anywhere gives
// Psi = 0 and zero gradient rows.  Everything is kept in named scalars (cf3 members), no indexed local arrays.
#pragma once
#include "geom_shared.h"
#include <stdint.h>

#pragma clang fp contract(off)

// IEEE-rounded on the host and on the device: hipcc compiles sqrtf and / correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt, which
// the build states).  Not __fsqrt_rn (csrc/surface_crossings_shared.h has the note).
#define CF_SQRT(a) sqrtf(a)

struct cf3 { float x, y, z; };

GEOM_FN cf3 cf_make(float x, float y, float z) { cf3 o; o.x = x, o.y = y, o.z = z; return o; }
GEOM_FN cf3 cf_load(const float *__restrict__ p) { return cf_make(p[0], p[1], p[2]); }
GEOM_FN cf3 cf_add(cf3 a, cf3 b) { return cf_make(a.x + b.x, a.y + b.y, a.z + b.z); }
GEOM_FN cf3 cf_sub(cf3 a, cf3 b) { return cf_make(a.x - b.x, a.y - b.y, a.z - b.z); }
GEOM_FN cf3 cf_scale(float s, cf3 a) { return cf_make(s * a.x, s * a.y, s * a.z); }
GEOM_FN cf3 cf_over(cf3 a, float s) { return cf_make(a.x / s, a.y / s, a.z / s); }
GEOM_FN float cf_dot(cf3 a, cf3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
GEOM_FN cf3 cf_cross(cf3 a, cf3 b) { return cf_make(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

struct CfConsts { float sigma, c0, c1, c2; };

GEOM_FN CfConsts cf_consts(float sigma)
{
    CfConsts k;
    const float s2 = 2.0f * sigma;
    k.sigma = sigma;
    k.c2 = (1.0f - s2) / (s2 * s2);
    k.c1 = 1.0f / s2;
    k.c0 = (3.0f - s2) / 4.0f;
    return k;
}

// What the evaluations and the reverse mode need of a receiver
struct CfRecord { cf3 a, e1, e2, N, n, u, v, q, o; float N2, len, d1, d2, den, r; };

GEOM_FN CfRecord cf_record(cf3 a, cf3 b, cf3 c)
{
    CfRecord R;
    R.a = a;
    R.e1 = cf_sub(b, a);
    R.e2 = cf_sub(c, a);
    R.N = cf_cross(R.e1, R.e2);
    R.N2 = cf_dot(R.N, R.N);
    R.len = CF_SQRT(R.N2);
    R.n = cf_over(R.N, R.len);
    R.d1 = cf_dot(R.e1, R.e1);
    R.d2 = cf_dot(R.e2, R.e2);
    R.u = cf_cross(R.e2, R.N);
    R.v = cf_cross(R.N, R.e1);
    const cf3 m = cf_add(cf_scale(R.d1, R.u), cf_scale(R.d2, R.v));
    R.den = 2.0f * R.N2;
    R.q = cf_over(m, R.den);
    R.o = cf_add(a, R.q);
    R.r = CF_SQRT(cf_dot(R.q, R.q));
    return R;
}

// One evaluation, and what its reverse mode reuses
struct CfEval { cf3 w, t; float h, rho, k1, D, Phi, Y, psi; bool active; };

GEOM_FN CfEval cf_eval(const CfRecord &R, const CfConsts &K, cf3 p)
{
    CfEval E;
    E.w = cf_sub(p, R.o);
    E.h = cf_dot(R.n, E.w);
    E.t = cf_sub(E.w, cf_scale(E.h, R.n));
    E.rho = CF_SQRT(cf_dot(E.t, E.t));
    E.k1 = 1.0f - E.h / K.sigma;
    E.D = R.r * E.k1;
    E.Phi = E.rho / E.D;
    E.Y = E.h <= -K.sigma ? (1.0f - E.h) - K.sigma : (K.c0 - K.c1 * E.h) - (K.c2 * E.h) * E.h;
    E.active = E.h < K.sigma && E.Phi < 1.0f;
    E.psi = E.active ? (1.0f - E.Phi) * E.Y : 0.0f;
    return E;
}

// energy of a (pair, role): the three penalties Psi^2 added in corner order
GEOM_FN float cf_energy(float p0, float p1, float p2) { return (p0 * p0 + p1 * p1) + p2 * p2; }

// The adjoints of a record, gathered over its three evaluations in corner order
struct CfAdjoint { cf3 n, o; float r; };

GEOM_FN CfAdjoint cf_adjoint_zero()
{
    CfAdjoint A;
    A.n = cf_make(0.0f, 0.0f, 0.0f), A.o = cf_make(0.0f, 0.0f, 0.0f), A.r = 0.0f;
    return A;
}

// Reverse mode of one evaluation for the upstream g2 = 2 g of its penalty Psi^2: returns the row of p and adds to the record's adjoints.
// t is perpendicular to n (|n| = 1), so rho does not depend on h through t, and the adjoint of n through t is -h t_bar.
GEOM_FN cf3 cf_eval_reverse(const CfRecord &R, const CfConsts &K, const CfEval &E, float g2, CfAdjoint *A)
{
    if (!E.active) return cf_make(0.0f, 0.0f, 0.0f);
    const float psi_b = g2 * E.psi;
    const float Phi_b = -(psi_b * E.Y);
    const float Y_b = psi_b * (1.0f - E.Phi);
    const float dY = E.h <= -K.sigma ? -1.0f : -K.c1 - (2.0f * K.c2) * E.h;
    const float rho_b = Phi_b / E.D;
    const float D_b = -(Phi_b * E.Phi) / E.D;
    const float r_b = D_b * E.k1;
    const float k1_b = D_b * R.r;
    const float h_b = Y_b * dY - k1_b / K.sigma;
    const cf3 t_b = E.rho > 0.0f ? cf_scale(rho_b / E.rho, E.t) : cf_make(0.0f, 0.0f, 0.0f);
    const cf3 w_b = cf_add(t_b, cf_scale(h_b, R.n));
    const cf3 n_b = cf_sub(cf_scale(h_b, E.w), cf_scale(E.h, t_b));
    A->n = cf_add(A->n, n_b);
    A->o = cf_sub(A->o, w_b);
    A->r = A->r + r_b;
    return w_b;
}

// Reverse mode of the record: the rows of its corners a, b, c from the gathered adjoints
GEOM_FN void cf_record_reverse(const CfRecord &R, const CfAdjoint &A, cf3 *ga, cf3 *gb, cf3 *gc)
{
    const cf3 q_b = R.r > 0.0f ? cf_add(A.o, cf_scale(A.r / R.r, R.q)) : A.o;
    const cf3 m_b = cf_over(q_b, R.den);
    const float den_b = -cf_dot(q_b, R.q) / R.den;
    const float N2_b = 2.0f * den_b;
    const float d1_b = cf_dot(m_b, R.u), d2_b = cf_dot(m_b, R.v);
    const cf3 u_b = cf_scale(R.d1, m_b), v_b = cf_scale(R.d2, m_b);
    cf3 e1_b = cf_add(cf_cross(v_b, R.N), cf_scale(2.0f * d1_b, R.e1));
    cf3 e2_b = cf_add(cf_cross(R.N, u_b), cf_scale(2.0f * d2_b, R.e2));
    cf3 N_b = cf_add(cf_cross(u_b, R.e2), cf_cross(R.e1, v_b));
    N_b = cf_add(N_b, cf_over(cf_sub(A.n, cf_scale(cf_dot(R.n, A.n), R.n)), R.len));
    N_b = cf_add(N_b, cf_scale(2.0f * N2_b, R.N));
    e1_b = cf_add(e1_b, cf_cross(R.e2, N_b));
    e2_b = cf_add(e2_b, cf_cross(N_b, R.e1));
    *gb = e1_b;
    *gc = e2_b;
    *ga = cf_sub(cf_sub(A.o, e1_b), e2_b);
}

// The (pair, role) statement: the three corners p0, p1, p2 of the intruder in the record of the receiver (a, b, c).  psi[3], the energy
// and, with rows != null, the six gradient rows for the upstream g (p0, p1, p2, a, b, c; 18 floats).  An evaluation that a gate closes
// adds nothing to the adjoints and has a zero row; a record none of whose evaluations is active is not reversed and has zero rows.
GEOM_FN float cf_pair_role(cf3 p0, cf3 p1, cf3 p2, cf3 a, cf3 b, cf3 c, const CfConsts &K, float g, float *__restrict__ psi,
                           float *__restrict__ rows)
{
    const CfRecord R = cf_record(a, b, c);
    const CfEval E0 = cf_eval(R, K, p0), E1 = cf_eval(R, K, p1), E2 = cf_eval(R, K, p2);
    psi[0] = E0.psi, psi[1] = E1.psi, psi[2] = E2.psi;
    if (rows) {
        const float g2 = 2.0f * g;
        CfAdjoint A = cf_adjoint_zero();
        const cf3 r0 = cf_eval_reverse(R, K, E0, g2, &A);
        const cf3 r1 = cf_eval_reverse(R, K, E1, g2, &A);
        const cf3 r2 = cf_eval_reverse(R, K, E2, g2, &A);
        cf3 ga = cf_make(0.0f, 0.0f, 0.0f), gb = ga, gc = ga;
        if (E0.active || E1.active || E2.active) cf_record_reverse(R, A, &ga, &gb, &gc);
        rows[0] = r0.x, rows[1] = r0.y, rows[2] = r0.z;
        rows[3] = r1.x, rows[4] = r1.y, rows[5] = r1.z;
        rows[6] = r2.x, rows[7] = r2.y, rows[8] = r2.z;
        rows[9] = ga.x, rows[10] = ga.y, rows[11] = ga.z;
        rows[12] = gb.x, rows[13] = gb.y, rows[14] = gb.z;
        rows[15] = gc.x, rows[16] = gc.y, rows[17] = gc.z;
    }
    return cf_energy(E0.psi, E1.psi, E2.psi);
}

// The aggregates, one (pair, role) entry after the other in pair order within a cell of pair_energy: role 0 of (i, j) belongs to E[i,j],
// role 1 to E[j,i]; a self pair adds (double) e0 + (double) e1 to E[i,i] at its role-0 entry and nothing at its role-1 entry.
GEOM_FN double cf_entry_value(int i, int j, int role, float e0, float e1)
{
    if (i != j) return (double)(role ? e1 : e0);
    return role ? 0.0 : (double)e0 + (double)e1;
}
