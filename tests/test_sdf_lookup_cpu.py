"""The fp64 reference of the SDF lookups (tests/sdf_lookup_ref.py) against independent statements of the same operation, and its
float32 coordinate emulation against its exact map.  No GPU: these anchor what tests/test_sdf_lookup_gpu.py compares the kernels with.

Volumes are iid U(-1, 1) (no symmetry, no smoothness), the boxes anisotropic and away from the origin, D in {2, 3, 5, 12}; the points
run from well outside the box to well inside it and include every node and the box corners themselves."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import psi_oracle as O
import sdf_lookup_ref as R

DIMS = [2, 3, 5, 12]
BOXES = [((0.7, -2.1, 3.3), (1.9, -0.4, 3.9)), ((-5.25, 0.031, -0.77), (-4.0, 2.6, -0.12))]
LEFT_OUT_CAP = 0.01
_cache = {}


def case(D, box):
    key = (D, box)
    if key not in _cache:
        gmin, gmax = np.asarray(BOXES[box][0], np.float32), np.asarray(BOXES[box][1], np.float32)
        vol = R.random_volume(100 + 7 * D + box, D)
        _cache[key] = (vol, gmin, gmax, points(gmin, gmax, D, 11 + D + box))
    return _cache[key]


def points(gmin, gmax, D, seed, n=6000):
    """uniform over the box enlarged by half its extent on every side (27 border classes, each well populated), every node of both
    conventions, gmin and gmax themselves, and their mixed corners"""
    rs = np.random.RandomState(seed)
    mn, mx = gmin.astype(np.float64), gmax.astype(np.float64)
    ext = mx - mn
    out = [rs.uniform(mn - 0.5 * ext, mx + 0.5 * ext, (n, 3))]
    for nodes in (np.arange(D) / (D - 1), (np.arange(D) + 0.5) / D):
        ax = [mn[a] + nodes * ext[a] for a in range(3)]
        out.append(np.stack(np.meshgrid(*ax, indexing='ij'), -1).reshape(-1, 3))
    out.append(np.stack(np.meshgrid(*[[mn[a], mx[a]] for a in range(3)], indexing='ij'), -1).reshape(-1, 3))
    return np.concatenate(out).astype(np.float32)


def grid_sample_64(vol, gmin, gmax, pts, ac):
    """torch.nn.functional.grid_sample in float64 on the float32 VALUES, gradient by autograd"""
    x = torch.tensor(pts.astype(np.float64), requires_grad=True)
    mn, mx = torch.tensor(gmin.astype(np.float64)), torch.tensor(gmax.astype(np.float64))
    nrm = (x - mn) / (mx - mn) * 2 - 1
    out = F.grid_sample(torch.tensor(vol.astype(np.float64))[None, None], nrm[:, [2, 1, 0]].view(1, -1, 1, 1, 3), padding_mode='border',
                        align_corners=ac).view(-1)
    out.sum().backward()
    return out.detach().numpy(), x.grad.numpy()


@pytest.mark.parametrize('ac', [True, False])
@pytest.mark.parametrize('box', [0, 1])
@pytest.mark.parametrize('D', DIMS)
def test_exact_lookup_is_grid_sample(D, box, ac):
    """fp64 against fp64: both sides round ~10 times at 2^-53.  The value agrees to 64 * 2^-53 * D (u carries D * 2^-53 of absolute
    error into slopes <= 2) everywhere; the gradient wherever the two fp64 u cannot fall into different cells: further than
    1e-9 of a cell from an integer (fp64 u errors are ~D * 1e-16); gmin and gmax themselves, exact borders, are checked for their zeros."""
    vol, gmin, gmax, pts = case(D, box)
    ex = R.exact_lookup(vol, gmin, gmax, pts, ac)
    val, grad = grid_sample_64(vol, gmin, gmax, pts, ac)
    assert np.abs(val - ex['value']).max() <= 64 * R.EPS64 * D * 4
    near = (np.abs(ex['u'] - np.rint(ex['u'])) < 1e-9).any(1)
    k = ((D - 1) if ac else D) / (gmax.astype(np.float64) - gmin.astype(np.float64))
    tol = 256 * R.EPS64 * D * k
    assert (np.abs(grad - ex['grad'])[~near] <= tol).all()
    assert (~near).mean() > 0.8
    # every one of the 27 (below | inside | above)^3 classes is populated, and a clamped axis has an exactly zero gradient
    cls = ex['cls']
    code = (cls[:, 0] + 1) * 9 + (cls[:, 1] + 1) * 3 + (cls[:, 2] + 1)
    assert np.bincount(code, minlength=27).min() >= 20
    assert (ex['grad'][cls != R.INSIDE] == 0).all() and (grad[~near][cls[~near] != R.INSIDE] == 0).all()
    # gmin / gmax themselves: clamped on every axis in both (u = 0, u = D - 1 exactly with align_corners; inside the half-cell margin without)
    corners = slice(len(pts) - 8, len(pts))
    assert (ex['cls'][corners] != R.INSIDE).all() and (ex['grad'][corners] == 0).all() and (grad[corners] == 0).all()


@pytest.mark.parametrize('ac', [True, False])
@pytest.mark.parametrize('D', DIMS)
def test_exact_lookup_is_the_oracle(D, ac):
    """oracle.psi_oracle.sdf_sample (float32 grid_sample behind the float32 normalisation): the operator's chain in the same order, so
    the operator's E_u and its interpolation allowance (sdf_lookup_ref: C_VALUE_OP, C_GRAD_OP; torch sums eight products of three
    weights: 3 products and a running sum per corner, no more roundings per unit of M than psi_trilinear's three stages)."""
    vol, gmin, gmax, pts = case(D, 0)
    ex = R.exact_lookup(vol, gmin, gmax, pts, ac)
    x = torch.tensor(pts[None], requires_grad=True)
    out = O.sdf_sample(torch.tensor(vol)[None], torch.tensor(gmin)[None], torch.tensor(gmax)[None], x, align_corners=ac).view(-1)
    out.sum().backward()
    eu = R.eu_operator(gmin, gmax, D, ac, pts)
    k = ((D - 1) if ac else D) / (gmax.astype(np.float64) - gmin.astype(np.float64))
    bv, bg = R.interp_bounds(np.ones(len(pts)), k, R.C_VALUE_OP, R.C_GRAD_OP)        # M <= 1: U(-1, 1)
    assert (np.abs(out.detach().numpy() - ex['value']) <= bv + R.transfer_bound(vol, eu)).all()
    keep = ~R.near_face(ex['u'], eu, D)
    assert 1.0 - keep.mean() <= 0.25, 'nodes are a fifth of these points; the uniform ones must stay'
    # within a cell the gradient along a moves with the OTHER axes' weights: their E_u times the mixed second differences (<= 2 steps)
    steps = R.node_steps(vol)
    mixed = np.stack([eu[:, [b for b in range(3) if b != a]].sum(1) * 2 * steps[a] * k[a] for a in range(3)], 1)
    assert (np.abs(x.grad.numpy()[0] - ex['grad'])[keep] <= (bg + mixed)[keep]).all()


@pytest.mark.parametrize('ac', [True, False])
@pytest.mark.parametrize('box', [0, 1])
@pytest.mark.parametrize('D', DIMS + [4, 16])
def test_cells_coords_within_eu(D, box, ac):
    gmin, gmax = np.asarray(BOXES[box][0], np.float32), np.asarray(BOXES[box][1], np.float32)
    pts = points(gmin, gmax, D, 5 + D)
    co = R.cells_coords(gmin, gmax, D, ac, pts)
    u = R.exact_u(gmin, gmax, D, ac, pts)
    eu = R.eu_cells(gmin, gmax, D, ac, pts)
    ratio = np.abs(co['u'].astype(np.float64) - u) / eu
    print('D=%d box=%d ac=%d: max |du| / E_u = %.3f, max E_u = %.2e cells' % (D, box, ac, ratio.max(), eu.max()))
    assert ratio.max() <= 1.0
    assert eu.max() < 1e-4, 'E_u is about 1e-5 of a cell at these boxes'
    # the statement's own consistency: cell + w is the clamped u, w in [0, 1), cell D - 1 only with w = 0
    assert (co['w'] >= 0).all() and (co['w'] < 1).all() and (co['cell'] >= 0).all() and (co['cell'] <= D - 1).all()
    assert (co['w'][co['cell'] == D - 1] == 0).all()
    assert np.array_equal(co['cell'] + co['w'].astype(np.float64), np.clip(co['u'].astype(np.float64), 0, D - 1))


@pytest.mark.parametrize('ac', [True, False])
@pytest.mark.parametrize('box', [0, 1])
@pytest.mark.parametrize('D', DIMS)
def test_cells_lookup_is_exact_lookup(D, box, ac):
    """value everywhere (continuity: E_u times the largest neighbouring-node difference, summed over the axes); gradient wherever no
    axis lies within E_u of an integer or a border, there within the other axes' E_u times the mixed differences plus the k rounding."""
    vol, gmin, gmax, _ = case(D, box)
    rs = np.random.RandomState(D * 31 + box)
    ext = gmax.astype(np.float64) - gmin.astype(np.float64)
    pts = rs.uniform(gmin - 0.5 * ext, gmax + 0.5 * ext, (20000, 3)).astype(np.float32)            # uniform points: the cap below is about them
    ex = R.exact_lookup(vol, gmin, gmax, pts, ac)
    ce = R.cells_lookup(vol, gmin, gmax, pts, ac)
    eu = R.eu_cells(gmin, gmax, D, ac, pts)
    assert (np.abs(ce['value'] - ex['value']) <= R.transfer_bound(vol, eu) + 16 * R.EPS64).all()
    left_out = R.near_face(ex['u'], eu, D)
    print('D=%d box=%d ac=%d: %d of %d points left out of the gradient comparison' % (D, box, ac, int(left_out.sum()), len(pts)))
    assert left_out.mean() <= LEFT_OUT_CAP
    keep = ~left_out
    assert np.array_equal(ce['inside'][keep], ex['cls'][keep] == R.INSIDE), 'away from the borders the float32 mask is the exact class'
    steps = R.node_steps(vol)
    kk = ce['k']
    k_true = ((D - 1) if ac else D) / ext
    mixed = np.stack([eu[:, [b for b in range(3) if b != a]].sum(1) * 2 * steps[a] * kk[a] for a in range(3)], 1)
    bound = mixed + np.abs(kk - k_true)[None, :] * steps[None, :] + 64 * R.EPS64 * kk[None, :]
    assert (np.abs(ce['grad'] - ex['grad'])[keep] <= bound[keep]).all()
    assert (ce['grad'][~ce['inside']] == 0).all()


def test_planted_nodes_and_borders():
    """cells_coords on points built to hit u = 0, an interior node and u = D - 1 exactly (power-of-two spacing, align_corners): the
    mask is strict at both borders, the interior node belongs to the UPPER cell with weight 0."""
    D, h = 8, 2.0 ** -4
    gmin = np.array([1.0, -3.0, 0.5], np.float32)
    gmax = (gmin + 7 * h).astype(np.float32)
    pts = np.stack([gmin, gmin + 3 * h, gmax]).astype(np.float32)
    co = R.cells_coords(gmin, gmax, D, True, pts)
    assert np.array_equal(co['u'], np.array([[0] * 3, [3] * 3, [7] * 3], np.float32))
    assert not co['inside'][0].any() and co['inside'][1].all() and not co['inside'][2].any()
    assert np.array_equal(co['cell'], [[0] * 3, [3] * 3, [7] * 3]) and (co['w'] == 0).all()
    vol = R.random_volume(3, D)
    ce = R.cells_lookup(vol, gmin, gmax, pts, True)
    v = vol.astype(np.float64)
    assert np.array_equal(ce['value'], [v[0, 0, 0], v[3, 3, 3], v[7, 7, 7]])
    assert np.array_equal(ce['grad'][1], np.array([v[4, 3, 3] - v[3, 3, 3], v[3, 4, 3] - v[3, 3, 3], v[3, 3, 4] - v[3, 3, 3]]) * ce['k'])
    assert (ce['grad'][[0, 2]] == 0).all()


def test_constants_are_derived_and_capped():
    assert R.C_VALUE <= 16 and R.C_GRAD <= 16
