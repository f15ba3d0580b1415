"""Two lanes per contact query in the NN search (nnindex_device.h: the template parameter LPQ) against four.

The width of a query's lane group changes how the work of one query is spread over lanes, never what is computed: the query point of the
fused engine's search role is blended by the same ascending-joint chains (fit.hip: ContactSkinSrc), every candidate is evaluated with the
same distance expression and compared by the same (distance, index) key, and the partial sums of a 64-query slice are formed by the
association of the 4-lane code (csrc/search_sum_order.h; tests/test_search_width_cpu.py walks that on the host).  So

  1. a fused engine created by default must equal one created under PSI_FIT_SEARCH_LANES=4 (and one under =2) BIT FOR BIT after 1 (cold: no
     hints), 2 and 12 (warm) iterations — the body vector, both Adam moments, the loss history, the hints, the slices fpart / gtc_part, the
     contact rows glc / gvpc / vpc and g_transl;
  2. the stand-alone operator of an index created under PSI_NN_SEARCH_LANES=2 must give the distances and indices of the brute-force
     psi_chamfer_forward bit for bit — cold, warm (hints of a call with the queries 1 cm away), with far hints (0.5 m away), for queries
     outside the cloud's box on one, two and three axes, on a cloud with duplicated points (lowest index wins) and for balls with more
     surviving columns than the scan's list holds (the tree walk with four child boxes per lane);
  3. repeated in the same process both give the same bits again.

Shapes: J = 55, V = 1100, m = 512, D = 16; n_c in {64, 65, 200}: one slice, a second slice with one query, a ragged last workgroup;
B in {1, 3, 33}.  Operator: n in {1, 63, 64, 65, 200}, m in {1, 7, 512}, B = 2."""
import copy
import dataclasses

import numpy as np
import pytest
import torch

from psi_release_amd import fitting, ops, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LOSS = {'weight_loss_rec': 1, 'weight_loss_vposer': 0.01, 'weight_contact': 0.1, 'weight_collision': 0.5}
V = 1100
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def scene(n_c, seed=0, dup=False):
    """make_scene at the test's size; dup: the first vertex of part 'butt' is ALSO the first of part 'back' — one vertex, two slots"""
    def make():
        s = synth.make_scene(seed, 512, 16, n_c, V=V)
        if dup:
            parts = copy.deepcopy(s.contact_parts)
            parts['butt']['verts_ind'][0] = parts['back']['verts_ind'][0]
            s = dataclasses.replace(s, contact_parts=parts)
            ids = synth.contact_ids_from_parts(parts)
            assert len(ids) == n_c and len(set(ids.tolist())) == n_c - 1
        return s
    return cached(('scene', n_c, seed, dup), make)


def make_op(scenes, B, **extra):
    cfg = {'scene_verts_path': None, 'scene_sdf_path': None, 'human_model_path': None, 'vposer_ckpt_path': None,
           'init_lr_h': 0.1, 'num_iter': 1, 'batch_size': B, 'device': torch.device(DEV),
           'contact_part': synth.CONTACT_PARTS, 'contact_id_folder': None, 'verbose': False,
           'smplx_data': cached('smplx', lambda: synth.make_smplx(7, V=V)), 'vposer_state': cached('vposer', lambda: synth.make_vposer_state(3)),
           'engine': 'fused', 'align_corners': True}
    cfg['scenes' if isinstance(scenes, (list, tuple)) else 'scene'] = list(scenes) if isinstance(scenes, (list, tuple)) else scenes
    cfg.update(extra)
    torch.manual_seed(0)
    return fitting.FittingOP(cfg, dict(LOSS))


def bodies_of(B):
    b = synth.make_bodies(21, B)
    b['cam_ext'] = synth.make_cam_ext(7, B)
    return b


def bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy()).view(np.uint32)


def run(scenes, B, n_c, lanes, monkeypatch, checkpoints=(1, 2, 12), slots=None, **extra):
    """The engine's state after each of `checkpoints` iterations as raw bits.  lanes: None (the default), 2 or 4 (PSI_FIT_SEARCH_LANES, read
    once when the engine is created)."""
    if lanes is None:
        monkeypatch.delenv('PSI_FIT_SEARCH_LANES', raising=False)
    else:
        monkeypatch.setenv('PSI_FIT_SEARCH_LANES', str(lanes))
    op = make_op(scenes, B, **extra)
    monkeypatch.delenv('PSI_FIT_SEARCH_LANES', raising=False)
    if slots is not None:
        op.set_scene_ids(slots)
    r = op.make_step_runner(bodies_of(B))
    eng, out, done = op._fused, [], 0
    nfp, ncp = (n_c + 63) // 64, (n_c + 255) // 256 * 256
    for n in checkpoints:
        r.steps(n - done)
        done = n
        x, hist, step = eng.read(n)
        assert step == n
        st = {'x': bits(x), 'adam_m': bits(eng.buffer('adam_m', (B, 75))), 'adam_v': bits(eng.buffer('adam_v', (B, 75))), 'losses': bits(hist),
              'nn_hint': bits(eng.buffer('nn_hint', (B, n_c))), 'fpart': bits(eng.buffer('fpart', (B, nfp))),
              'gtc_part': bits(eng.buffer('gtc_part', (B, nfp, 4)))[:, :, :3], 'g_transl': bits(eng.buffer('g_transl', (B, 3))),
              'gA': bits(eng.buffer('gA', (B, 64, 16))), 'gfeat': bits(eng.buffer('gfeat', (B, 512)))}
        for name in ('glc', 'gvpc', 'vpc'):
            st[name] = bits(eng.buffer(name, (B, 3 * ncp)))[:, :3 * n_c]
        out.append(st)
    hint = out[0]['nn_hint'].view(np.int32)
    assert ((hint >= 0) & (hint < 512)).all(), 'a query without a winner after the first iteration'
    return out


def assert_same_bits(a, b, what):
    for i, (sa, sb) in enumerate(zip(a, b)):
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), '%s: %s differs at checkpoint %d (%d of %d words)' % (what, k, i, int((sa[k] != sb[k]).sum()), sa[k].size)


def compare_widths(scenes, B, n_c, monkeypatch, what, **kw):
    four = run(scenes, B, n_c, 4, monkeypatch, **kw)
    assert_same_bits(run(scenes, B, n_c, None, monkeypatch, **kw), four, what + ', default against 4 lanes')
    two = run(scenes, B, n_c, 2, monkeypatch, **kw)
    assert_same_bits(two, four, what + ', 2 lanes against 4')
    return two


# ---- 1. fused engines --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 3, 33])
@pytest.mark.parametrize('n_c', [64, 65, 200])
def test_fused_engine_two_lanes_equal_four(monkeypatch, n_c, B):
    compare_widths(scene(n_c), B, n_c, monkeypatch, 'n_c=%d B=%d' % (n_c, B))


def test_a_contact_vertex_listed_twice(monkeypatch):
    compare_widths(scene(65, dup=True), 3, 65, monkeypatch, 'duplicate contact vertex')


def test_independent_bodies(monkeypatch):
    compare_widths(scene(200), 3, 200, monkeypatch, 'independent bodies', independent_bodies=True)


def test_two_scenes(monkeypatch):
    """psi_fit_create_scenes: the several-scenes instance of the launch follows the same decision"""
    B = 3
    scenes = [scene(65), dataclasses.replace(scene(65), verts=scene(65, seed=5).verts)]
    compare_widths(scenes, B, 65, monkeypatch, 'two scenes', slots=np.asarray([1, 0, 1], np.int32))


def test_fused_engine_repeats_its_bits(monkeypatch):
    """3. the same engine kind twice in one process"""
    a = run(scene(200), 3, 200, 2, monkeypatch)
    assert_same_bits(run(scene(200), 3, 200, 2, monkeypatch), a, '2 lanes, second engine')


# ---- 2. the operator against brute force ---------------------------------------------------------------------------------------------
def index(cloud, lanes, monkeypatch):
    """SceneNNIndex created under PSI_NN_SEARCH_LANES (read where the index is created)"""
    if lanes == 2:
        monkeypatch.setenv('PSI_NN_SEARCH_LANES', '2')
    else:
        monkeypatch.delenv('PSI_NN_SEARCH_LANES', raising=False)
    ix = ops.SceneNNIndex(cloud, DEV)
    monkeypatch.delenv('PSI_NN_SEARCH_LANES', raising=False)
    return ix


def brute(q, cloud):
    """psi_chamfer_forward, query side: (dist bits, idx)"""
    c = torch.as_tensor(cloud, device=DEV)[None].expand(q.shape[0], -1, -1).contiguous()
    d, i, _, _ = ops.chamfer_forward_raw(q, c, both=False)
    return bits(d), i.cpu().numpy()


def check_query(ix, q, cloud, hint, what):
    d, i = ix.query(q, hint)
    bd, bi = brute(q, cloud)
    gd, gi = bits(d), i.cpu().numpy()
    assert np.array_equal(gi, bi), '%s: %d of %d indices differ from brute force' % (what, int((gi != bi).sum()), gi.size)
    assert np.array_equal(gd, bd), '%s: %d of %d distances differ from brute force' % (what, int((gd != bd).sum()), gd.size)
    if hint is not None:
        assert np.array_equal(hint.cpu().numpy(), bi), what + ': the hints are not the winners'
    return gd, gi


def cloud_of(m, seed=3, dup=False):
    rs = np.random.RandomState(seed)
    c = rs.uniform(-1.5, 1.5, (m, 3)).astype(np.float32)
    if dup and m >= 4:
        c[m // 2:] = c[:m - m // 2]                # every point of the second half repeats one of the first: the lower index must win
    return c


def queries(n, B=2, seed=9, scale=1.4):
    rs = np.random.RandomState(seed)
    return torch.as_tensor(rs.uniform(-scale, scale, (B, n, 3)).astype(np.float32), device=DEV)


@pytest.mark.parametrize('lanes', [2, 4])
@pytest.mark.parametrize('m', [1, 7, 512])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 200])
def test_operator_equals_brute_force(monkeypatch, n, m, lanes):
    for dup in (False, True):
        cloud = cloud_of(m, dup=dup)
        ix = index(cloud, lanes, monkeypatch)
        q = queries(n)
        what = 'n=%d m=%d lanes=%d dup=%d' % (n, m, lanes, dup)
        cold = check_query(ix, q, cloud, None, what + ' cold')
        for name, shift in (('warm', 0.01), ('far hints', 0.5)):
            hint = torch.full((q.shape[0], n), -1, dtype=torch.int32, device=DEV)
            moved = q + torch.as_tensor([shift, 0.0, 0.0], device=DEV)
            check_query(ix, moved, cloud, hint, what + ' ' + name + ' (the call that leaves the hints)')
            check_query(ix, q, cloud, hint, what + ' ' + name)
        # outside the cloud's box on one, two and three axes, cold and with the hints of the inside queries' neighbours
        for axes in ((0,), (0, 2), (0, 1, 2)):
            off = np.zeros(3, np.float32)
            off[list(axes)] = (2.5, -1.9, 3.25)[:len(axes)]
            out = q * 0.3 + torch.as_tensor(off, device=DEV)
            hint = torch.full((q.shape[0], n), -1, dtype=torch.int32, device=DEV)
            check_query(ix, out, cloud, hint, what + ' outside on %d axes, cold' % len(axes))
            check_query(ix, out + 0.01, cloud, hint, what + ' outside on %d axes, warm' % len(axes))
        # 3. again, in the same process
        again = check_query(ix, q, cloud, None, what + ' cold, repeated')
        assert np.array_equal(again[0], cold[0]) and np.array_equal(again[1], cold[1])


def surviving_columns(cloud, q, best):
    """The scan's candidate and surviving column counts of a ball (nnindex_device.h: kd_query_round), restated in fp32 for queries inside the box:
    (ncand, nsurv) per query"""
    f = np.float32
    m = cloud.shape[0]
    mn, mx = cloud.min(0), cloud.max(0)
    ext = (mx - mn).astype(np.float64)
    h = max(np.cbrt(np.prod(np.maximum(ext, 1e-3 * ext.max())) * 2.5 / m), ext.max() / 128.0)
    ginv = f(1.0 / h)
    gn = np.minimum(128, np.maximum(1, np.floor((mx - mn) * ginv).astype(int) + 1))
    ru = np.sqrt(best.astype(f)) * ginv * f(1.0001) + f(0.01)
    uq = (q - mn) * ginv
    res = []
    for k in range(q.shape[0]):
        lo = np.clip(np.floor(uq[k, :2] - ru[k]), 0, gn[:2] - 1).astype(int)
        hi = np.clip(np.floor(uq[k, :2] + ru[k]), 0, gn[:2] - 1).astype(int)
        ncand, nsurv = int(np.prod(hi - lo + 1)), 0
        for cx in range(lo[0], hi[0] + 1):
            for cy in range(lo[1], hi[1] + 1):
                dx = max(cx - uq[k, 0], uq[k, 0] - cx - 1, 0)
                dy = max(cy - uq[k, 1], uq[k, 1] - cy - 1, 0)
                nsurv += ru[k] * ru[k] - dx * dx - dy * dy >= 0
        res.append((ncand, int(nsurv)))
    return res


@pytest.mark.parametrize('lanes', [2, 4])
def test_ball_with_more_columns_than_the_list(monkeypatch, lanes):
    """A cloud of 4096 points (a 12 x 12 x 12 grid of cells) with an empty ball in the middle; warm queries near its centre have balls of
    radius 3 - 4.5 cells: more than GRID_LIST_MAX = 48 surviving columns (or more than 64 candidates) — the tree walk, four child boxes per
    lane with two lanes per query."""
    rs = np.random.RandomState(4)
    full = rs.uniform(-1.5, 1.5, (6000, 3)).astype(np.float32)
    n_long = 0
    for R in (0.8, 0.95, 1.1):
        cloud = full[np.linalg.norm(full, axis=1) > R][:4096]
        assert cloud.shape[0] == 4096
        ix = index(cloud, lanes, monkeypatch)
        q = torch.as_tensor(rs.uniform(-0.12, 0.12, (2, 65, 3)).astype(np.float32), device=DEV)
        hint = torch.full((2, 65), -1, dtype=torch.int32, device=DEV)
        check_query(ix, q + 0.004, cloud, hint, 'hole %.2f lanes=%d (the call that leaves the hints)' % (R, lanes))
        hp = cloud[hint.cpu().numpy().reshape(-1)]
        qn = q.cpu().numpy().reshape(-1, 3)
        counts = surviving_columns(cloud, qn, ((hp - qn) ** 2).sum(1))
        n_long += sum(1 for nc, ns in counts if ns > 48 or nc > 64)
        check_query(ix, q, cloud, hint, 'hole %.2f lanes=%d warm' % (R, lanes))
    print('%d warm queries with more than 48 surviving columns or more than 64 candidates' % n_long)
    assert n_long >= 65, 'the holes do not produce long column lists: broken test'
