"""CPU checks of the several-scenes fitting engine's boundary: exported symbols, the ctypes scene struct against the header, and the
pure-Python planner of packed runs across scenes."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


@pytest.fixture(scope='module')
def built_lib():
    from psi_release_amd import build
    path = build.build()
    assert os.path.exists(path)
    return path


def test_library_exports_the_scene_entry_points(built_lib):
    from psi_release_amd import build, hip
    for path in (built_lib, build.LIB_FMA):
        lib = ctypes.CDLL(path)
        for name in ('psi_fit_create_scenes', 'psi_fit_set_scene_slots', 'psi_fit_scene_count'):
            assert hasattr(lib, name), '%s does not export %s' % (os.path.basename(path), name)
            assert name in hip.SIGNATURES
    # psi_fit_create with S scenes instead of the four single-scene arguments: 13 shared arguments + table + count
    assert len(hip.SIGNATURES['psi_fit_create_scenes'][1]) == len(hip.SIGNATURES['psi_fit_create'][1]) - 4 + 2


def test_fit_scene_struct_matches_header():
    """`hip.FitScene` (ctypes) must list the fields of `struct psi_fit_scene` (include/psi_hip.h) with the same names, order and types."""
    from psi_release_amd import hip
    text = open(os.path.join(ROOT, 'include', 'psi_hip.h')).read()
    body = re.search(r'typedef struct psi_fit_scene \{(.*?)\} psi_fit_scene;', text, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.rsplit(None, 1) if '*' in decl else decl.split(None, 1)
        for nm in names.split(','):
            nm = nm.strip()
            if nm.startswith('*'):
                fields.append((nm[1:], ctype + ' *'))
            elif '[' in nm:
                fields.append((nm[:nm.index('[')], '%s[%s]' % (ctype, nm[nm.index('[') + 1:nm.index(']')])))
            else:
                fields.append((nm, ctype))
    want = {'int': ctypes.c_int, 'const float *': ctypes.c_void_p, 'float[3]': ctypes.c_float * 3}
    got = list(hip.FitScene._fields_)
    assert [n for n, _ in got] == [n for n, _ in fields] == ['d_verts', 'd_sdf', 'm', 'D', 'gmin', 'gmax']
    assert all(t is want[c] for (_, t), (_, c) in zip(got, fields))
    assert ctypes.sizeof(hip.FitScene) == 2 * ctypes.sizeof(ctypes.c_void_p) + 2 * 4 + 6 * 4


@pytest.mark.parametrize('counts,pack', [((3, 0, 5), 4), ((0, 0, 0), 4), ((1,), 4), ((4, 4), 4), ((2, 7, 0, 1), 3), ((5, 2), 1)])
def test_plan_runs_on_ragged_work_lists(counts, pack):
    from psi_release_amd.run_plan import plan_runs
    work = [['s%d_f%d' % (s, i) for i in range(n)] for s, n in enumerate(counts)]
    records, runs = plan_runs(work, pack)
    n = sum(counts)
    assert records == [r for lst in work for r in lst]
    assert len(runs) == (n + pack - 1) // pack and all(len(run) == pack for run in runs)
    flat = [pair for run in runs for pair in run]
    # every record exactly once before the padding, in its own scene's slot
    assert [i for i, _ in flat[:n]] == list(range(n))
    assert all(0 <= s < len(counts) and records[i] in work[s] for i, s in flat)
    # padding only in the last run: copies of its last real pair
    assert all(pair == flat[n - 1] for pair in flat[n:]) and len(flat) - n < pack
    for run in runs[:-1]:
        assert len(set(i for i, _ in run)) == pack
    with pytest.raises(ValueError):
        plan_runs(work, 0)
