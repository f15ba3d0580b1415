"""Seeded synthetic assets with the shapes of the licensed PSI inputs.

None of the assets the reference needs ship with it (SMPL-X ``SMPLX_NEUTRAL.npz``,
VPoser ``vposer_v1_0``, PROX-E scenes, ``data/resnet18.pth`` are licensed or
missing blobs; reference README.md:76-111, .MISSING_LARGE_BLOBS:1), so parity
tests, the oracle's golden fixtures and ``bench.py`` all draw from this module.
Everything uses ``numpy.random.RandomState`` (bit-stable across numpy versions
and machines) so the GPU box regenerates exactly what the fixtures were made
from; ``tests/golden/manifest.json`` pins checksums.

Shapes follow SURVEY.md section 8: V=10475 vertices, J=55 joints, 486 pose
blendshape rows, 20 shape components (10 betas + 10 expression), 12 hand PCA
components.
"""
from __future__ import annotations

import hashlib
import json
import os
from dataclasses import dataclass, field

import numpy as np

V_SMPLX = 10475
J_SMPLX = 55
NB_SMPLX = 20
N_HAND_PCA = 12

# SMPL-X kinematic tree (public model topology: pelvis, hips/spine, ..., jaw, eyes,
# 15 left-hand and 15 right-hand joints hanging off the wrists 20 / 21).
SMPLX_PARENTS = np.array(
    [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 15, 15, 15,
     20, 25, 26, 20, 28, 29, 20, 31, 32, 20, 34, 35, 20, 37, 38,
     21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50, 21, 52, 53], dtype=np.int64)

CONTACT_PARTS = ['back', 'butt', 'L_Hand', 'R_Hand', 'L_Leg', 'R_Leg', 'thighs']


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def checksum(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


@dataclass
class SMPLXData:
    """Arrays with the keys/shapes of ``SMPLX_NEUTRAL.npz`` that the path uses."""
    v_template: np.ndarray          # [V,3]
    shapedirs: np.ndarray           # [V,3,NB]  (10 betas | 10 expression)
    posedirs: np.ndarray            # [V,3,486] (npz layout; body model reshapes to [486,3V])
    J_regressor: np.ndarray         # [J,V]
    weights: np.ndarray             # [V,J]
    kintree_table: np.ndarray       # [2,J] row 0 = parents
    hands_componentsl: np.ndarray   # [45,45] (first 12 rows used)
    hands_componentsr: np.ndarray
    hands_meanl: np.ndarray         # [45]
    hands_meanr: np.ndarray
    f: np.ndarray                   # [F,3] faces (unused on the hot path)

    def save_npz(self, path: str) -> None:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.savez(path, **self.__dict__)


def make_smplx(seed: int = 7, V: int = V_SMPLX, J: int = J_SMPLX, parents: np.ndarray | None = None,
               nb: int = NB_SMPLX, weight_nnz: int = 0) -> SMPLXData:
    """SMPL-X-shaped model: peaky (approximately sparse) regressor / skinning weights.  ``weight_nnz`` > 0: every vertex is bound to
    exactly that many joints — a joint and its neighbours in the kinematic tree, consecutive vertices mostly to the same joint —
    as in the released SMPL-X model, whose skinning rows have at most 4 non-zeros (the default is a DENSE random [V, J] matrix,
    which is what the reference's dense matmul is indifferent to and the harder case for this package's kernels)."""
    rs = np.random.RandomState(seed)
    if parents is None:
        parents = SMPLX_PARENTS if J == J_SMPLX else np.array([-1] + [(i - 1) // 2 for i in range(1, J)])
    v_template = _f32(rs.standard_normal((V, 3)) * 0.3)
    shapedirs = _f32(rs.standard_normal((V, 3, nb)) * 0.01)
    posedirs = _f32(rs.standard_normal((V, 3, (J - 1) * 9)) * 0.001)
    jr = rs.uniform(0, 1, (J, V)) ** 8
    J_regressor = _f32(jr / jr.sum(1, keepdims=True))
    w = rs.uniform(0, 1, (V, J)) ** 8
    if weight_nnz > 0:
        par = np.asarray(parents)
        nbrs = [[j] + ([int(par[j])] if par[j] >= 0 else []) + [int(c) for c in np.nonzero(par == j)[0]] for j in range(J)]
        prim = np.minimum((np.arange(V) * J) // V, J - 1)                      # consecutive vertices share their primary joint
        mask = np.zeros((V, J), bool)
        for v in range(V):
            cand = list(nbrs[int(prim[v])])
            while len(cand) < weight_nnz:                                      # leaves: widen to the neighbours' neighbours
                cand += [c for q in list(cand) for c in nbrs[q] if c not in cand] or [int(rs.randint(J))]
            mask[v, cand[:weight_nnz]] = True
        w = np.where(mask, w + 1e-3, 0.0)
    weights = _f32(w / w.sum(1, keepdims=True))
    kintree = np.stack([parents.astype(np.int64), np.arange(J, dtype=np.int64)])
    kintree[0, 0] = -1
    hcl = _f32(rs.standard_normal((45, 45)) * 0.3)
    hcr = _f32(rs.standard_normal((45, 45)) * 0.3)
    hml = _f32(rs.standard_normal(45) * 0.1)
    hmr = _f32(rs.standard_normal(45) * 0.1)
    faces = rs.randint(0, V, (64, 3)).astype(np.int64)
    return SMPLXData(v_template, shapedirs, posedirs, J_regressor, weights, kintree, hcl, hcr, hml, hmr, faces)


def make_vposer_state(seed: int = 3, num_neurons: int = 512, latentD: int = 32, n_joints: int = 21) -> dict:
    """``VPoser(512, 32, [1,21,3])`` state_dict (numpy), keys as vposer_smpl.py:75-89.

    Linear layers use U(-1/sqrt(fan_in), 1/sqrt(fan_in)) like ``nn.Linear``'s default
    reset; BatchNorm buffers are at their defaults.  Only the ``dec`` half is on the path.
    """
    rs = np.random.RandomState(seed)
    nf = n_joints * 3

    def lin(out_f, in_f, gain=1.0):
        k = gain / np.sqrt(in_f)
        return _f32(rs.uniform(-k, k, (out_f, in_f))), _f32(rs.uniform(-k, k, (out_f,)))

    sd = {}
    for name, n in (('bodyprior_enc_bn1', nf), ('bodyprior_enc_bn2', num_neurons)):
        sd[name + '.weight'] = np.ones(n, np.float32)
        sd[name + '.bias'] = np.zeros(n, np.float32)
        sd[name + '.running_mean'] = np.zeros(n, np.float32)
        sd[name + '.running_var'] = np.ones(n, np.float32)
        sd[name + '.num_batches_tracked'] = np.zeros((), np.int64)
    for name, (o, i) in (('bodyprior_enc_fc1', (num_neurons, nf)), ('bodyprior_enc_fc2', (num_neurons, num_neurons)),
                         ('bodyprior_enc_mu', (latentD, num_neurons)), ('bodyprior_enc_logvar', (latentD, num_neurons)),
                         ('bodyprior_dec_fc1', (num_neurons, latentD)), ('bodyprior_dec_fc2', (num_neurons, num_neurons)),
                         ('bodyprior_dec_out', (n_joints * 6, num_neurons))):
        # decoder gain > 1 so that random latents give well-spread joint rotations
        w, b = lin(o, i, gain=2.0 if 'dec' in name else 1.0)
        sd[name + '.weight'], sd[name + '.bias'] = w, b
    return sd


@dataclass
class SceneData:
    verts: np.ndarray        # [m,3] downsampled scene point cloud (scenes_downsampled/*.ply vertices)
    sdf: np.ndarray          # [D,D,D] indexed [ix][iy][iz] (C order, fitting_proxe.py:85)
    grid_min: np.ndarray     # [3]
    grid_max: np.ndarray     # [3]
    grid_dim: int
    contact_parts: dict = field(default_factory=dict)  # part -> {'verts_ind': [...], 'faces_ind': [...]}

    def write_prox_layout(self, root: str, name: str = 'S') -> dict:
        """Write the on-disk formats the entry points read (fitting_proxe.py:80-96, cvae.py:99-115)."""
        os.makedirs(os.path.join(root, 'scenes_sdf'), exist_ok=True)
        os.makedirs(os.path.join(root, 'scenes_downsampled'), exist_ok=True)
        os.makedirs(os.path.join(root, 'body_segments'), exist_ok=True)
        with open(os.path.join(root, 'scenes_sdf', name + '.json'), 'w') as f:
            json.dump({'min': self.grid_min.tolist(), 'max': self.grid_max.tolist(), 'dim': int(self.grid_dim)}, f)
        np.save(os.path.join(root, 'scenes_sdf', name + '_sdf.npy'), self.sdf.reshape(-1))
        write_ply_vertices(os.path.join(root, 'scenes_downsampled', name + '.ply'), self.verts)
        for part, d in self.contact_parts.items():
            with open(os.path.join(root, 'body_segments', part + '.json'), 'w') as f:
                json.dump(d, f)
        return {'scene_verts_path': os.path.join(root, 'scenes_downsampled', name + '.ply'),
                'scene_sdf_path': os.path.join(root, 'scenes_sdf', name),
                'contact_id_folder': os.path.join(root, 'body_segments')}


def make_scene(seed: int = 0, m: int = 32768, D: int = 256, n_contact: int = 2048, V: int = V_SMPLX,
               extent: float = 2.0, radius: float = 0.8, kind: str = 'room') -> SceneData:
    """One scene: m points U(-1.5,1.5)^3, an analytic SDF on [-extent,extent]^3, contact ids in 7 part files.

    kind='room'  : sdf = radius - |p|  (free space inside a spherical room, walls penetrate) - a
                   minority of body vertices is negative, like a body touching PROX furniture;
    kind='sphere': sdf = |p| - radius  (solid ball at the origin; the survey's planning scene)."""
    rs = np.random.RandomState(seed)
    verts = _f32(rs.uniform(-1.5, 1.5, (m, 3)))
    ax = np.linspace(-extent, extent, D, dtype=np.float32)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing='ij')
    rr = np.sqrt(X * X + Y * Y + Z * Z)
    sdf = (np.float32(radius) - rr if kind == 'room' else rr - np.float32(radius)).astype(np.float32)
    ids = np.sort(rs.choice(V, n_contact, replace=False))
    parts = {}
    for name, p in zip(CONTACT_PARTS, np.array_split(ids, len(CONTACT_PARTS))):
        parts[name] = {'verts_ind': [int(x) for x in p], 'faces_ind': [0]}
    return SceneData(verts, sdf, np.array([-extent] * 3, np.float32), np.array([extent] * 3, np.float32), D, parts)


def contact_ids_from_parts(parts: dict, order=CONTACT_PARTS) -> np.ndarray:
    """Same expression as GeometryTransformer.get_contact_id (cvae.py:99-115): list(set(.)) per part, concatenated."""
    return np.concatenate([list(set(parts[p]['verts_ind'])) for p in order]).astype(np.int64)


def make_bodies(seed: int = 11, B: int = 32) -> dict:
    """Generated-body pkl contents (keys of cvae.py:320-327) in the scale the survey specifies."""
    rs = np.random.RandomState(seed)
    return {
        'transl': _f32(rs.standard_normal((B, 3)) * 0.3),
        'global_orient': _f32(rs.standard_normal((B, 3)) * 0.5),
        'betas': _f32(rs.standard_normal((B, 10))),
        'body_pose': _f32(rs.standard_normal((B, 32))),
        'left_hand_pose': _f32(rs.standard_normal((B, 12)) * 0.3),
        'right_hand_pose': _f32(rs.standard_normal((B, 12)) * 0.3),
        'cam_ext': _f32(np.tile(np.eye(4)[None], (B, 1, 1))),
        'cam_int': _f32(np.tile(np.array([[1000., 0, 960.], [0, 1000., 540.], [0, 0, 1.]])[None], (B, 1, 1))),
    }


def make_cam_ext(seed: int = 5, B: int = 32) -> np.ndarray:
    """Random rigid camera-to-world transforms [B,4,4] (non-identity cam_ext exercises verts_transform)."""
    rs = np.random.RandomState(seed)
    out = np.tile(np.eye(4, dtype=np.float64)[None], (B, 1, 1))
    for b in range(B):
        q, _ = np.linalg.qr(rs.standard_normal((3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        out[b, :3, :3] = q
        out[b, :3, 3] = rs.standard_normal(3) * 0.2
    return _f32(out)


def body_vector_72(bodies: dict) -> np.ndarray:
    """[transl|global_orient|betas|vposer latent|lh|rh] = 72-D (cvae.py:312-319)."""
    return _f32(np.concatenate([bodies[k] for k in
                                ('transl', 'global_orient', 'betas', 'body_pose', 'left_hand_pose', 'right_hand_pose')], -1))


from .scene_io import read_ply_vertices, write_ply_vertices  # noqa: E402,F401


def make_state_like(shapes: dict, seed: int = 0) -> dict:
    """Synthetic state_dict for a module given {key: shape}: per-key generators (order independent), nn-style scales.

    Used for the CVAE models, whose pretrained weights (``data/resnet18.pth``, PSI checkpoints) are licensed / missing."""
    import zlib
    out = {}
    for key, shape in shapes.items():
        rs = np.random.RandomState((zlib.crc32(key.encode()) ^ (seed * 2654435761)) & 0x7fffffff)
        shape = tuple(shape)
        if key.endswith('num_batches_tracked'):
            out[key] = np.zeros(shape, np.int64)
        elif key.endswith('running_var'):
            out[key] = _f32(rs.uniform(0.5, 1.5, shape))
        elif key.endswith('running_mean'):
            out[key] = _f32(rs.standard_normal(shape) * 0.1)
        elif len(shape) == 1 and ('bn' in key or '.1.weight' in key or 'downsample.1' in key) and key.endswith('weight'):
            out[key] = _f32(rs.uniform(0.5, 1.5, shape))
        elif len(shape) == 1:
            out[key] = _f32(rs.uniform(-0.05, 0.05, shape))
        else:
            fan_in = int(np.prod(shape[1:]))
            k = 1.0 / np.sqrt(fan_in)
            out[key] = _f32(rs.uniform(-k, k, shape))
    return out


def make_cvae_inputs(seed: int = 13, B: int = 4) -> dict:
    """Scene images (depth | semantics in [-1,1], [B,2,128,128]), body vectors and reparameterisation noise."""
    rs = np.random.RandomState(seed)
    return {'xs': _f32(rs.uniform(-1, 1, (B, 2, 128, 128))),
            'x75': _f32(rs.standard_normal((B, 75)) * 0.5),
            'eps32': _f32(rs.standard_normal((B, 32))),
            'eps32b': _f32(rs.standard_normal((B, 32)))}


@dataclass
class RoomMesh:
    verts: np.ndarray        # [nv,3] fp32, z up, the floor at z = 0
    faces: np.ndarray        # [nf,3] int32; the first n_room_faces are the closed room box
    labels: np.ndarray       # [nv] fp32 semantic label per vertex (mpcat40-style ids, 0..41)
    n_room_faces: int
    box_min: np.ndarray      # [3] the room box
    box_max: np.ndarray

    def without_room(self) -> 'RoomMesh':
        """The furniture and the free triangles alone (a camera outside then sees background pixels)."""
        return RoomMesh(self.verts, np.ascontiguousarray(self.faces[self.n_room_faces:]), self.labels, 0, self.box_min, self.box_max)

    def rgb(self) -> np.ndarray:
        """Vertex colours that ``scene_io.labels_from_colors`` maps back to round(labels): grey = 5 * label."""
        return np.repeat(np.clip(np.rint(self.labels * 5.0), 0, 255).astype(np.uint8)[:, None], 3, axis=1)

    def planes(self) -> np.ndarray:
        """[6,2,3]: (point, inward normal) of the six room planes, the ``room_planes`` of ``rendering.sample_virtual_cams``."""
        c = 0.5 * (self.box_min.astype(np.float64) + self.box_max)
        out = []
        for ax in range(3):
            for side, sgn in ((self.box_min, 1.0), (self.box_max, -1.0)):
                p, n = c.copy(), np.zeros(3)
                p[ax], n[ax] = side[ax], sgn
                out.append(np.stack([p, n]))
        return np.stack(out)


def _quad_grid(p0, du, dv, k):
    """(k+1)^2 vertices and 2 k^2 triangles of the parallelogram p0 + s du + t dv, s, t in [0,1]."""
    s = np.linspace(0.0, 1.0, k + 1)
    S, T = np.meshgrid(s, s, indexing='ij')
    v = p0[None, None] + S[..., None] * du[None, None] + T[..., None] * dv[None, None]
    idx = np.arange((k + 1) * (k + 1)).reshape(k + 1, k + 1)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    return v.reshape(-1, 3), np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], 0)


def _box_quads(lo, hi):
    """The six faces of an axis-aligned box as (p0, du, dv, axis, side)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    quads = []
    for ax in range(3):
        u, v = (ax + 1) % 3, (ax + 2) % 3
        du, dv = np.zeros(3), np.zeros(3)
        du[u], dv[v] = hi[u] - lo[u], hi[v] - lo[v]
        for side in (0, 1):
            p0 = lo.copy()
            p0[ax] = hi[ax] if side else lo[ax]
            quads.append((p0, du, dv, ax, side))
    return quads


def make_room_mesh(seed: int = 0, n_extra: int = 180, subdiv: int = 1, extra_size: float = 0.6) -> RoomMesh:
    """Stand-in scene mesh: a closed 5 x 4 x 2.6 m box room (walls 1, floor 2, ceiling 17), three labelled furniture boxes standing on
    the floor, and ``n_extra`` random free triangles of edge ~``extra_size`` that intersect each other and the furniture, with a random
    label per VERTEX (so labels vary inside a triangle).  ``subdiv`` = k cuts every box face into 2 k^2 triangles (k = 64 gives
    ~197 k triangles for timing); the default is 12 + 36 + n_extra triangles."""
    rs = np.random.RandomState(seed)
    lo, hi = np.array([-2.5, -2.0, 0.0]), np.array([2.5, 2.0, 2.6])
    verts, faces, labels = [], [], []
    nv = 0

    def add_box(blo, bhi, label_of):
        nonlocal nv
        for p0, du, dv, ax, side in _box_quads(blo, bhi):
            v, f = _quad_grid(p0, du, dv, subdiv)
            verts.append(v)
            faces.append(f + nv)
            labels.append(np.full(len(v), label_of(ax, side), np.float64))
            nv += len(v)

    add_box(lo, hi, lambda ax, side: 1.0 if ax < 2 else (17.0 if side else 2.0))
    n_room = sum(len(f) for f in faces)
    for label in (3.0, 5.0, 10.0):                                   # chair, table, sofa
        size = rs.uniform([0.5, 0.5, 0.4], [1.4, 1.0, 1.0])
        ctr = rs.uniform(lo[:2] + 0.9, hi[:2] - 0.9)
        blo = np.array([ctr[0] - size[0] / 2, ctr[1] - size[1] / 2, 0.0])
        add_box(blo, blo + size, lambda ax, side, label=label: label)
    if n_extra:
        c = rs.uniform(lo + 0.3, hi - 0.3, (n_extra, 3))
        tri = c[:, None, :] + rs.uniform(-extra_size / 2, extra_size / 2, (n_extra, 3, 3))
        verts.append(np.clip(tri.reshape(-1, 3), lo + 0.02, hi - 0.02))
        faces.append(np.arange(3 * n_extra).reshape(n_extra, 3) + nv)
        labels.append(rs.randint(0, 42, 3 * n_extra).astype(np.float64))
    return RoomMesh(_f32(np.concatenate(verts)), np.ascontiguousarray(np.concatenate(faces), dtype=np.int32), _f32(np.concatenate(labels)),
                    n_room, _f32(lo), _f32(hi))


def make_room_cams(which: str = 'inside') -> np.ndarray:
    """Camera-to-world poses [n,4,4] fp64 for ``make_room_mesh``: 'inside' = three cameras in the room looking at a point above the floor
    (parts of the walls lie behind each of them, so the near clip runs), 'outside' = one camera 7 m away looking at the room's centre."""
    from .rendering import look_at
    target = np.array([0.2, -0.1, 0.9])
    if which == 'inside':
        eyes = [[-2.1, -1.6, 1.7], [2.0, 1.5, 2.2], [1.9, -1.7, 1.2]]
    else:
        eyes = [[-6.0, -4.5, 3.4]]
    return np.stack([look_at(np.array(e), target) for e in eyes])


def make_capsule_mesh(n_ring: int = 12, n_seg: int = 16, r: float = 0.16, h: float = 1.7):
    """Stand-in body surface (``make_smplx``'s vertices are a random cloud with random faces): a closed capsule of radius ``r`` and height
    ``h`` along z with its base at z = 0.  Two pole vertices and ``n_ring - 1`` rings of ``n_seg`` vertices at the polar angles
    pi * i / n_ring: those up to the equator on the sphere around (0, 0, r), those above it on the sphere around (0, 0, h - r), so the band
    between the two middle rings is the (slightly conical) trunk; faces wound outwards.  Returns (verts [V,3] fp32, faces [F,3] int32),
    V = 2 + (n_ring - 1) * n_seg, F = 2 * n_seg * (n_ring - 1): 178 and 352."""
    if n_ring < 3 or n_seg < 3 or h <= 2 * r:
        raise ValueError('a capsule needs n_ring >= 3, n_seg >= 3 and h > 2 r')
    theta = np.pi * np.arange(1, n_ring) / n_ring
    phi = 2.0 * np.pi * np.arange(n_seg) / n_seg
    zc = np.where(theta <= np.pi / 2 + 1e-12, r, h - r)
    ring = np.stack([r * np.sin(theta)[:, None] * np.cos(phi)[None], r * np.sin(theta)[:, None] * np.sin(phi)[None],
                     np.broadcast_to((zc - r * np.cos(theta))[:, None], (n_ring - 1, n_seg))], -1)
    verts = np.concatenate([[[0.0, 0.0, 0.0]], ring.reshape(-1, 3), [[0.0, 0.0, h]]])
    idx = 1 + np.arange((n_ring - 1) * n_seg).reshape(n_ring - 1, n_seg)
    nxt = np.roll(idx, -1, axis=1)
    top = len(verts) - 1
    faces = [np.stack([np.zeros(n_seg, np.int64), nxt[0], idx[0]], 1)]
    for i in range(n_ring - 2):
        faces += [np.stack([idx[i], nxt[i], nxt[i + 1]], 1), np.stack([idx[i], nxt[i + 1], idx[i + 1]], 1)]
    faces.append(np.stack([np.full(n_seg, top), idx[-1], nxt[-1]], 1))
    return _f32(verts), np.ascontiguousarray(np.concatenate(faces), dtype=np.int32)


@dataclass
class OrientedRoom:
    """A closed, consistently oriented stand-in scene with an exact distance field (``make_oriented_room``)."""
    verts: np.ndarray        # [nv,3] fp32, per-face vertices (unwelded)
    faces: np.ndarray        # [nf,3] int32; every triangle faces free space
    box_min: np.ndarray      # [3] the room box
    box_max: np.ndarray
    boxes: list              # (centre [3], half sizes [3], rotation [3,3]) of the solids in the room, fp64

    def analytic_sdf(self, points) -> np.ndarray:
        """Signed distance (fp64) of points [..., 3] to the scene the mesh describes before its vertices were rounded to fp32: positive in
        the free space of the room, negative inside a box and outside the room.  The minimum of the room-interior distance and the box
        distances, which is exact because the solids are disjoint."""
        p = np.asarray(points, np.float64)

        def box_sdf(q):                                           # q = |local p| - half sizes
            return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0)

        c, h = 0.5 * (self.box_min.astype(np.float64) + self.box_max), 0.5 * (self.box_max.astype(np.float64) - self.box_min)
        out = -box_sdf(np.abs(p - c) - h)
        for centre, half, rot in self.boxes:
            out = np.minimum(out, box_sdf(np.abs((p - centre) @ rot) - half))
        return out


def make_oriented_room(subdiv: int = 2) -> OrientedRoom:
    """The 5 x 4 x 2.6 m room box of ``make_room_mesh`` oriented inward, an axis-aligned box [0.3,1.5] x [-1.2,-0.4] x [0.05,0.8] and a box
    of half sizes (0.5, 0.3, 0.4) rotated 30 degrees about z and centred at (-1.0, 0.7, 0.5), both oriented outward and floating 5 cm above
    the floor (no coincident surfaces).  Every face is cut into 2 subdiv^2 triangles with vertices of its own, rounded to fp32: welding
    them gives a closed manifold whose every triangle faces free space, the convention of a signed distance volume (free space positive).
    ``subdiv`` = 64 gives ~147 k triangles for timing."""
    lo, hi = np.array([-2.5, -2.0, 0.0]), np.array([2.5, 2.0, 2.6])
    ang = np.radians(30.0)
    rot = np.array([[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]])
    solids = [(np.array([0.9, -0.8, 0.425]), np.array([0.6, 0.4, 0.375]), np.eye(3)),
              (np.array([-1.0, 0.7, 0.5]), np.array([0.5, 0.3, 0.4]), rot)]
    verts, faces = [], []
    nv = 0
    for centre, half, R, outward in [(0.5 * (lo + hi), 0.5 * (hi - lo), np.eye(3), False)] + [s + (True,) for s in solids]:
        for p0, du, dv, ax, side in _box_quads(-half, half):
            v, f = _quad_grid(p0, du, dv, subdiv)                  # its triangles face +axis
            if bool(side) != outward:
                f = f[:, ::-1]
            verts.append(v @ R.T + centre)
            faces.append(f + nv)
            nv += len(v)
    return OrientedRoom(_f32(np.concatenate(verts)), np.ascontiguousarray(np.concatenate(faces), dtype=np.int32), _f32(lo), _f32(hi), solids)


def make_open_room(subdiv: int = 2, drop_ceiling: bool = True, sink: float = 0.0) -> OrientedRoom:
    """``make_oriented_room`` with the defects of real scans: the ceiling triangles removed (``drop_ceiling``: the mesh is open, 4 subdiv
    edges of the walls lose their second triangle) and/or the first, axis-aligned box lowered by ``sink`` metres (0.05: it stands exactly
    on the floor, two coincident and oppositely oriented surfaces; more: it interpenetrates the floor).  The faces keep the order of
    ``make_oriented_room``; ``analytic_sdf`` is that of the closed room with the moved box (where the box reaches below the floor the
    minimum over the solids still has the right sign, which is what it is used for)."""
    room = make_oriented_room(subdiv)
    nq, nt = (subdiv + 1) ** 2, 2 * subdiv * subdiv              # vertices and triangles per box face
    centre, half, rot = room.boxes[0]
    moved = (centre - np.array([0.0, 0.0, float(sink)]), half, rot)
    verts = room.verts.copy()
    box = [_quad_grid(p0, du, dv, subdiv)[0] @ rot.T + moved[0] for p0, du, dv, _, _ in _box_quads(-half, half)]
    verts[6 * nq:12 * nq] = _f32(np.concatenate(box))
    faces = room.faces
    if drop_ceiling:                                             # the sixth face of the room box: axis 2, upper side
        faces = np.ascontiguousarray(np.concatenate([faces[:5 * nt], faces[6 * nt:]]))
    return OrientedRoom(verts, faces, room.box_min, room.box_max, [moved] + list(room.boxes[1:]))


def flip_faces(faces, fraction: float, seed: int = 0):
    """(faces, mask): a copy of ``faces`` [nf,3] with columns 1 and 2 swapped in a seeded subset of round(fraction * nf) triangles (their
    normals reversed), and the bool mask [nf] of that subset: a mesh with mixed winding, the input of ``scene_sdf.orient_faces``."""
    f = np.array(faces, copy=True).reshape(-1, 3)
    if not 0.0 <= fraction <= 1.0:
        raise ValueError('fraction lies in [0, 1]')
    mask = np.zeros(len(f), bool)
    mask[np.random.RandomState(seed).permutation(len(f))[:int(round(fraction * len(f)))]] = True
    f[mask] = f[mask][:, [0, 2, 1]]
    return f, mask
