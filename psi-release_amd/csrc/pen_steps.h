// The penetration mask (FitDev::penmask, fit.hip) as the blend backward reads it: bits are VERTICES, the stream walks 16-COLUMN STEPS of
// the [V][3] gradient rows.  Step s is columns 16 s .. 16 s + 15, i.e. vertices floor(16 s / 3) .. floor((16 s + 15) / 3) — five or six
// of them, in one mask word or straddling two.  No dependencies: tools/pen_steps_host_check.hip runs these statements on the host.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PSI_PEN_HD __host__ __device__
#else
#define PSI_PEN_HD
#endif

PSI_PEN_HD inline int psi_pen_step_first_vertex(int s) { return (16 * s) / 3; }
PSI_PEN_HD inline int psi_pen_step_last_vertex(int s) { return (16 * s + 15) / 3; }

// the mask words [w0, w0 + nw) that the steps [s_begin, s_end) touch (s_end > s_begin); a word is 64 vertices
PSI_PEN_HD inline void psi_pen_step_words(int s_begin, int s_end, int &w0, int &nw)
{
    w0 = psi_pen_step_first_vertex(s_begin) >> 6;
    nw = (psi_pen_step_last_vertex(s_end - 1) >> 6) - w0 + 1;
}

// true when a vertex owning one of step s's columns has its bit set.  vm[j] is mask word w0 + j for j in [0, nw): bit i = vertex
// 64 (w0 + j) + i; vertices outside those words count as clear (the rows' padding beyond the mask)
PSI_PEN_HD inline bool psi_pen_step_live(const unsigned long long *vm, int w0, int nw, int s)
{
    const int v_lo = psi_pen_step_first_vertex(s), v_hi = psi_pen_step_last_vertex(s);
    const int j_lo = (v_lo >> 6) - w0, j_hi = (v_hi >> 6) - w0;
    const unsigned long long from = ~0ull << (v_lo & 63), upto = ~0ull >> (63 - (v_hi & 63));
    if (j_lo == j_hi) return j_lo >= 0 && j_lo < nw && (vm[j_lo] & from & upto) != 0ull;
    return (j_lo >= 0 && j_lo < nw && (vm[j_lo] & from) != 0ull) || (j_hi >= 0 && j_hi < nw && (vm[j_hi] & upto) != 0ull);
}
