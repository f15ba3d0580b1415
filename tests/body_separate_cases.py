"""The cases shared by tests/test_body_separate_cpu.py and tests/test_body_separate_gpu.py: the inputs of the three kernels (random G at the
chunk boundaries), the loops on the capsule batches of tests/body_overlap_cases.py and on ``thin`` of tests/surface_crossings_cases.py with
their pinned iteration counts, and the host-check plumbing.  Every reference is computed once, shared and read-only."""
import subprocess

import numpy as np

import body_overlap_cases as BC
import body_separate_ref as R
import surface_crossings_cases as SC

CAP = 40                # iterations within which a loop must have separated its batch: a condition, not a measurement
# What the fp32 restatement needs (tests/test_body_separate_cpu.py asserts them): the loop with its defaults (sigma = 0.5, 'depth'), with
# body 0 held fixed, with penalty='squared' and sigma = 1e-3, with w_cross = 0 (which stops with PAIRS_LEFT crossing pairs), and on thin
ITERATIONS = {'c12x16': 11, 'c12x16_fixed0': 12, 'c12x16_squared': 13, 'c12x16_pen_only': 10, 'thin': 8}
ITERATIONS_C24X46 = 21  # the restatement's count, taken once (81 s of NumPy: the GPU test holds the batch to CAP + 4, as the loop's contract says)
PAIRS_LEFT = 88
UNTOUCHED = (2, 3)      # bodies of c12x16 no iteration finds a triple or a pair for (body 4 starts clear and is pushed into later)
LOOPS = {'c12x16': {}, 'c12x16_fixed0': dict(fixed=[0]), 'c12x16_squared': dict(penalty='squared', sigma=1e-3),
         'c12x16_pen_only': dict(w_cross=0.0), 'thin': {}}
STEPS = 10
KERNEL_CASES = [(V, B) for V in (178, 256, 257, 1060) for B in (1, 6)]
ZERO_BODY, FIXED_BODY = 2, 4        # of the B = 6 kernel cases: a body whose G is zero (delta == 0 at every step) and a fixed one
_KERNEL, _LOOPS = {}, {}


U = 2.0 ** -24          # the unit roundoff of fp32


def pose_bound(base, pivot, transl):
    """|x32 - x64| per coordinate, both forms on the same fp32 inputs, to first order in U and with 1 % for the higher orders.  With D the
    largest |d| component and |R_kl| <= 1 (+ a few U):
        an entry of R      two products, a sum or difference, the doubling (exact), for the diagonal one more difference:  <= 4 U
        d = base - pivot   one rounding: <= U D, carried through R unamplified, three terms                                 <= 3 U D
        R_kl d_l           the entry's error times D, three terms: 12 U D; the three products' own roundings               <= 3 U D
        the two sums       partial sums of at most 2 D and 3 D                                                              <= 5 U D
        p = pivot + transl one rounding, <= U |p|; the last sum, <= U |x|
    together U (23 D + |p| + |x|)."""
    D = np.abs(base.astype(np.float64) - pivot[:, None]).max()
    P = np.abs(pivot.astype(np.float64) + transl).max()
    return 1.01 * U * (23.0 * D + P + (3.0 * D + P))


def loop_inputs(name):
    if name == 'thin':
        c = SC.case('thin')
    else:
        c = BC.case('c12x16')
    return c.verts, c.faces


def loop(name):
    """(state, verts, iterations, separated, trace) of R.separate on the named loop, max_iter = CAP."""
    if name not in _LOOPS:
        base, faces = loop_inputs(name)
        _LOOPS[name] = R.separate(base, faces, max_iter=CAP, **LOOPS[name])
    return _LOOPS[name]


class KernelCase:
    """base [B,V,3], pivot, G [STEPS,B,V,3], fixed (a list or None) and the restatement's rehearsal of the STEPS steps."""

    def __init__(self, V, B):
        rng = np.random.default_rng(1000 * V + B)
        if V in (178, 1060):
            self.base = np.ascontiguousarray(BC.case('c12x16' if V == 178 else 'c24x46').verts[:B])
        else:
            self.base = (rng.normal(size=(B, V, 3)) * 0.4 + rng.normal(size=(B, 1, 3))).astype(np.float32)
        assert self.base.shape == (B, V, 3)
        self.pivot = R.default_pivot(self.base)
        self.G = (rng.normal(size=(STEPS, B, V, 3)) * 10.0 ** rng.integers(-4, 1, size=(STEPS, B, 1, 1))).astype(np.float32)
        self.fixed = None
        if B > FIXED_BODY:
            self.G[:, ZERO_BODY] = 0
            self.fixed = [FIXED_BODY]
        self.steps = rehearse(self.base, R.State(B, self.pivot), self.G, self.fixed)
        for a in (self.base, self.pivot, self.G):
            a.setflags(write=False)


def rehearse(base, state, G, fixed=None, **kw):
    """Per step k = 1 .. len(G): dict(verts, chunks, g6, state) with ``state`` the State after the step; ``before`` the one it posed."""
    out = []
    for k, Gk in enumerate(G, 1):
        verts = R.pose(base, state.quat, state.transl, state.pivot)
        chunks = R.chunk_sums(R.wrench_terms(verts, Gk, state.pivot + state.transl))
        g6 = R.g6_of(chunks)
        after = R.step(state, g6, k, fixed=fixed, **kw)
        out.append(dict(verts=verts, chunks=chunks, g6=g6, before=state, state=after))
        state = after
    return out


def kernel_case(V, B):
    if (V, B) not in _KERNEL:
        _KERNEL[(V, B)] = KernelCase(V, B)
    return _KERNEL[(V, B)]


def write_batch(path, base, state, G, fixed, lr_t=0.01, lr_r=0.01, betas=(0.9, 0.999), eps=1e-8):
    B, V = base.shape[:2]
    with open(path, 'wb') as f:
        f.write(np.array([B, V, len(G), 0 if fixed is None else 1], np.int32).tobytes())
        f.write(np.array([lr_t, lr_r, betas[0], betas[1], eps], np.float64).tobytes())
        for a in (base, state.pivot, state.quat, state.transl, state.m, state.s):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
        if fixed is not None:
            f.write(np.isin(np.arange(B), fixed).astype(np.int32).tobytes())
        f.write(np.ascontiguousarray(G, np.float32).tobytes())


def run_host_check(exe, tmp, base, state, G, fixed=None, **kw):
    """The steps of tools/body_separate_host_check.hip built as ``exe``: a list of dict(verts, chunks, g6, quat, transl, m, s)."""
    src, out = str(tmp / 'batch.bin'), str(tmp / 'out.bin')
    write_batch(src, base, state, G, fixed, **kw)
    r = subprocess.run([exe, src, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, 'rb').read()
    B, V = base.shape[:2]
    nchunk = (V + R.CHUNK - 1) // R.CHUNK
    at = [0]

    def take(dtype, shape):
        a = np.frombuffer(raw, dtype, int(np.prod(shape)), at[0]).reshape(shape)
        at[0] += a.nbytes
        return a

    steps = [dict(verts=take(np.float32, (B, V, 3)), chunks=take(np.float64, (B, nchunk, 6)), g6=take(np.float32, (B, 6)),
                  quat=take(np.float32, (B, 4)), transl=take(np.float32, (B, 3)), m=take(np.float32, (B, 6)), s=take(np.float32, (B, 6)))
             for _ in range(len(G))]
    assert at[0] == len(raw)
    return steps


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_step(got, want, what=''):
    """``got``: dict(verts, chunks, g6, quat, transl, m, s) of a host-check or GPU step; ``want``: a step of ``rehearse``."""
    for k in ('verts', 'chunks', 'g6'):
        if k in got:
            assert same_bits(got[k], want[k]), (what, k)
    for k in ('quat', 'transl', 'm', 's'):
        assert same_bits(got[k], getattr(want['state'], k)), (what, k)
