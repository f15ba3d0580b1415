"""On-disk formats of a PROX-E / MP3D-R scene as the fitting entry points read them.

* ``{scene_sdf_path}.json`` (``min``, ``max``, ``dim``) + ``{scene_sdf_path}_sdf.npy`` (flat D^3 fp32, C order x,y,z)
  — fitting_proxe.py:80-85
* ``scenes_downsampled/{scene}.ply`` vertices — fitting_proxe.py:93-96 (the reference uses open3d; only the vertex
  positions are consumed, so a small PLY vertex reader replaces that dependency)
* ``body_segments/{part}.json`` — cvae.py:99-115 (see geometry.GeometryTransformer.get_contact_id)
"""
from __future__ import annotations

import json

import numpy as np


def read_sdf(scene_sdf_path: str):
    with open(scene_sdf_path + '.json') as f:
        d = json.load(f)
    grid_min = np.array(d['min'], dtype=np.float32)
    grid_max = np.array(d['max'], dtype=np.float32)
    dim = int(d['dim'])
    sdf = np.load(scene_sdf_path + '_sdf.npy').reshape(dim, dim, dim).astype(np.float32)
    return sdf, grid_min, grid_max, dim


_PLY_TYPES = {'float': '<f4', 'float32': '<f4', 'double': '<f8', 'float64': '<f8', 'uchar': 'u1', 'uint8': 'u1',
              'char': 'i1', 'int8': 'i1', 'short': '<i2', 'int16': '<i2', 'ushort': '<u2', 'uint16': '<u2',
              'int': '<i4', 'int32': '<i4', 'uint': '<u4', 'uint32': '<u4'}


def read_ply_vertices(path: str) -> np.ndarray:
    """Vertex positions [m,3] fp32 of an ASCII or binary-little-endian PLY."""
    with open(path, 'rb') as f:
        header = []
        while True:
            line = f.readline()
            if not line:
                raise ValueError('PLY header not terminated: %s' % path)
            header.append(line.decode('ascii', 'replace').strip())
            if header[-1] == 'end_header':
                break
        fmt = [h for h in header if h.startswith('format')][0].split()[1]
        nvert, props, in_vertex = 0, [], False
        for h in header:
            t = h.split()
            if t[:2] == ['element', 'vertex']:
                nvert, in_vertex = int(t[2]), True
            elif t and t[0] == 'element':
                in_vertex = False
            elif t and t[0] == 'property' and in_vertex:
                props.append((t[1], t[2]))
        names = [p[1] for p in props]
        if fmt == 'ascii':
            ix = [names.index(c) for c in 'xyz']
            rows = np.array([f.readline().split() for _ in range(nvert)], dtype=np.float64)
            return np.ascontiguousarray(rows[:, ix], dtype=np.float32)
        if fmt != 'binary_little_endian':
            raise ValueError('unsupported PLY format %s' % fmt)
        dt = np.dtype([(n, _PLY_TYPES[t]) for t, n in props])
        arr = np.frombuffer(f.read(nvert * dt.itemsize), dtype=dt, count=nvert)
        return np.ascontiguousarray(np.stack([arr['x'], arr['y'], arr['z']], -1), dtype=np.float32)


def write_ply_vertices(path: str, verts: np.ndarray) -> None:
    verts = np.ascontiguousarray(verts, dtype=np.float32)
    with open(path, 'wb') as f:
        f.write(b'ply\nformat binary_little_endian 1.0\n')
        f.write(('element vertex %d\n' % len(verts)).encode())
        f.write(b'property float x\nproperty float y\nproperty float z\nelement face 0\n'
                b'property list uchar int vertex_indices\nend_header\n')
        f.write(verts.tobytes())


def _ply_header(f, path):
    """(format, [(element name, count, [(kind, ...)])]) of an open PLY; a property is ('scalar', type, name) or
    ('list', count type, item type, name)."""
    if f.readline().strip() != b'ply':
        raise ValueError('not a PLY file: %s' % path)
    fmt, elements = None, []
    while True:
        line = f.readline()
        if not line:
            raise ValueError('PLY header not terminated: %s' % path)
        t = line.decode('ascii', 'replace').split()
        if not t or t[0] in ('comment', 'obj_info'):
            continue
        if t[0] == 'end_header':
            return fmt, elements
        if t[0] == 'format':
            fmt = t[1]
        elif t[0] == 'element':
            elements.append((t[1], int(t[2]), []))
        elif t[0] == 'property':
            elements[-1][2].append(('list', t[2], t[3], t[4]) if t[1] == 'list' else ('scalar', t[1], t[2]))


def labels_from_colors(rgb) -> np.ndarray:
    """Per-vertex semantic label of an MP3D-style coloured mesh: min(mean(rgb) / 5, 41), rgb in 0..255 — the value
    utils_prox_snapshots_virtualcam.py:57-58 derives before it truncates to an integer id."""
    return np.minimum(np.asarray(rgb, dtype=np.float64).mean(-1) / 5.0, 41.0).astype(np.float32)


def read_ply_mesh(path: str):
    """(verts [nv,3] fp32, faces [nf,3] int32, rgb [nv,3] uint8 or None) of an ASCII or binary-little-endian PLY with triangle faces
    (``vertex_indices`` / ``vertex_index`` list) and optional ``red`` / ``green`` / ``blue`` vertex properties."""
    with open(path, 'rb') as f:
        fmt, elements = _ply_header(f, path)
        if fmt not in ('ascii', 'binary_little_endian'):
            raise ValueError('unsupported PLY format %s' % fmt)
        verts = rgb = None
        faces = np.zeros((0, 3), np.int32)
        for name, count, props in elements:
            lists = [p for p in props if p[0] == 'list']
            if name == 'vertex':
                if lists:
                    raise ValueError('list property in the vertex element: %s' % path)
                names = [p[2] for p in props]
                if fmt == 'ascii':
                    rows = np.array([f.readline().split() for _ in range(count)], dtype=np.float64).reshape(count, len(names))
                    col = lambda n: rows[:, names.index(n)]
                else:
                    dt = np.dtype([(p[2], _PLY_TYPES[p[1]]) for p in props])
                    arr = np.frombuffer(f.read(count * dt.itemsize), dtype=dt, count=count)
                    col = lambda n: arr[n]
                verts = np.ascontiguousarray(np.stack([col(c) for c in 'xyz'], -1), dtype=np.float32)
                if all(c in names for c in ('red', 'green', 'blue')):
                    rgb = np.ascontiguousarray(np.stack([col(c) for c in ('red', 'green', 'blue')], -1)).astype(np.uint8)
            elif name == 'face':
                if len(lists) != 1 or lists[0][3] not in ('vertex_indices', 'vertex_index'):
                    raise ValueError('expected one vertex_indices list per face: %s' % path)
                if fmt == 'ascii':
                    k = props.index(lists[0])                       # scalar properties before the list shift its column
                    rows = [f.readline().split() for _ in range(count)]
                    if any(int(r[k]) != 3 for r in rows):
                        raise ValueError('only triangle faces are supported: %s' % path)
                    faces = np.array([r[k + 1:k + 4] for r in rows], dtype=np.int64).reshape(count, 3).astype(np.int32)
                else:
                    fields = []
                    for p in props:                                 # a triangle-only face element has fixed-size rows
                        if p[0] == 'list':
                            fields += [('_n', _PLY_TYPES[p[1]]), ('_i', _PLY_TYPES[p[2]], (3,))]
                        else:
                            fields.append((p[2], _PLY_TYPES[p[1]]))
                    dt = np.dtype(fields)
                    arr = np.frombuffer(f.read(count * dt.itemsize), dtype=dt, count=count)
                    if (arr['_n'] != 3).any():
                        raise ValueError('only triangle faces are supported: %s' % path)
                    faces = np.ascontiguousarray(arr['_i']).astype(np.int32)
            elif count:
                raise ValueError('unsupported PLY element %s: %s' % (name, path))
        if verts is None:
            raise ValueError('no vertex element: %s' % path)
        return verts, faces, rgb


def write_ply_mesh(path: str, verts: np.ndarray, faces: np.ndarray, rgb=None, ascii: bool = False) -> None:
    """Triangle mesh (+ optional uint8 vertex colours) as a binary-little-endian (default) or ASCII PLY that ``read_ply_mesh`` reads."""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    if rgb is not None:
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8).reshape(len(verts), 3)
    head = 'ply\nformat %s 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n' % (
        'ascii' if ascii else 'binary_little_endian', len(verts))
    if rgb is not None:
        head += 'property uchar red\nproperty uchar green\nproperty uchar blue\n'
    head += 'element face %d\nproperty list uchar int vertex_indices\nend_header\n' % len(faces)
    with open(path, 'wb') as f:
        f.write(head.encode())
        if ascii:
            for i, v in enumerate(verts):
                row = ' '.join(repr(float(x)) for x in v)
                if rgb is not None:
                    row += ' %d %d %d' % tuple(int(c) for c in rgb[i])
                f.write((row + '\n').encode())
            for t in faces:
                f.write(('3 %d %d %d\n' % tuple(int(i) for i in t)).encode())
            return
        vdt = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')] + ([('red', 'u1'), ('green', 'u1'), ('blue', 'u1')] if rgb is not None else [])
        va = np.zeros(len(verts), dtype=np.dtype(vdt))
        va['x'], va['y'], va['z'] = verts[:, 0], verts[:, 1], verts[:, 2]
        if rgb is not None:
            va['red'], va['green'], va['blue'] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
        f.write(va.tobytes())
        fa = np.zeros(len(faces), dtype=np.dtype([('n', 'u1'), ('i', '<i4', (3,))]))
        fa['n'], fa['i'] = 3, faces
        f.write(fa.tobytes())
