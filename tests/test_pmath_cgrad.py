"""CPU tests of the trainable curvature: the seven _c entry points exist in the library, the header and the ctypes table
within ABI version 15, they refuse by name without a launch, and the fixture tests/golden/pmath_cgrad.npz holds every case with the
reference's own fp32 c gradient within the bound of its float64 one."""
import ctypes
import os

import numpy as np

from pmath_cgrad_cases import BOUND, EDGE_OPS, EDGE_ROWS, MODULES, PAIR_SHAPES, ROW_OPS, ROW_SHAPES, cases, err
from pmath_vjp_cases import DIST_MATRIX, MATVEC
from test_capi_symbols import header_functions

NEW = {'sttode_pmath_rowop_c': 9, 'sttode_pmath_matvec_c': 10, 'sttode_pmath_pair_c': 10, 'sttode_pmath_rowop_bwd_c': 12,
       'sttode_pmath_matvec_bwd_c': 15, 'sttode_pmath_dist_matrix_bwd_c': 12, 'sttode_pmath_hsoftmax_bwd_c': 15}


def test_library_header_and_table_agree_on_the_new_entry_points():
    from sttode_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = ctypes.CDLL(capi.LIB_PATH)
    fns = header_functions()
    for name, nargs in NEW.items():
        assert hasattr(L, name), name + ' is not exported'
        assert name in fns and len(fns[name]) == nargs, (name, fns.get(name))
        assert len(capi.SIGNATURES[name]) == nargs
        for ct, decl in zip(capi.SIGNATURES[name], fns[name]):
            assert (ct is ctypes.c_int and decl.startswith('int ')) or (ct is ctypes.c_void_p and '*' in decl), (name, decl)
        assert sum('c_dev' in decl for decl in fns[name]) == 1 and not any(decl.startswith('float c') for decl in fns[name]), name
    assert L.sttode_abi_version() == capi.ABI_VERSION == 15


def test_new_entry_points_refuse_by_name_without_a_launch():
    """Argument checks come first and name the entry point (host only: nothing is launched, no GPU needed)."""
    from sttode_amd import capi
    L = capi.lib()
    one = ctypes.c_void_p(8)          # never dereferenced: every call below fails its checks

    def refused(name, word, *args):
        assert getattr(L, name)(*args) != 0, (name, word)
        msg = L.sttode_last_error().decode()
        assert name + ':' in msg and word in msg, msg
    # a NULL c_dev, every entry point
    refused('sttode_pmath_rowop_c', 'c_dev', 2, one, one, one, None, 4, 4, None, None)
    refused('sttode_pmath_matvec_c', 'c_dev', one, one, one, one, one, 4, 4, 4, None, None)
    refused('sttode_pmath_pair_c', 'c_dev', 0, one, one, None, one, 4, 4, 4, None, None)
    refused('sttode_pmath_rowop_bwd_c', 'c_dev', 2, one, one, one, one, one, 4, 4, None, one, one, None)
    refused('sttode_pmath_matvec_bwd_c', 'c_dev', one, one, one, one, one, one, one, one, 4, 4, 4, None, one, one, None)
    refused('sttode_pmath_dist_matrix_bwd_c', 'c_dev', one, one, one, one, one, 4, 4, 4, None, one, one, None)
    refused('sttode_pmath_hsoftmax_bwd_c', 'c_dev', one, one, one, one, one, one, one, one, 4, 4, 4, None, one, one, None)
    # the other refusals
    for op, word in ((12, 'unknown op'), (13, 'unknown op'), (99, 'unknown op'), (-1, 'unknown op')):
        refused('sttode_pmath_rowop_c', word, op, one, one, one, None, 4, 4, one, None)
    refused('sttode_pmath_rowop_c', 'second operand', 2, one, None, one, None, 4, 4, one, None)
    refused('sttode_pmath_pair_c', 'needs A', 2, one, one, None, one, 4, 4, 4, one, None)
    for op, y, gy, word in ((12, one, None, 'Oblique'), (13, one, None, 'internal'), (99, one, None, 'unknown op'), (2, None, None, 'second operand'),
                            (0, None, one, 'gy')):
        refused('sttode_pmath_rowop_bwd_c', word, op, one, y, one, one, gy, 4, 4, one, one, one, None)
    refused('sttode_pmath_rowop_bwd_c', 'gc_ws', 2, one, one, one, one, one, 4, 4, one, None, one, None)
    refused('sttode_pmath_rowop_bwd_c', 'gc_ws', 2, one, one, one, one, one, 4, 4, one, one, None, None)
    refused('sttode_pmath_matvec_bwd_c', 'gmx_ws', one, one, one, one, None, None, one, None, 4, 4, 4, one, one, one, None)
    refused('sttode_pmath_matvec_bwd_c', 'gc_ws', one, one, one, one, one, None, one, one, 4, 4, 4, one, None, one, None)
    refused('sttode_pmath_dist_matrix_bwd_c', 'gc_ws', one, one, one, one, one, 4, 4, 4, one, None, one, None)
    refused('sttode_pmath_dist_matrix_bwd_c', 'positive', one, one, one, one, one, 0, 4, 4, one, one, one, None)
    refused('sttode_pmath_hsoftmax_bwd_c', 'together', one, one, one, one, one, one, one, None, 4, 4, 4, one, one, one, None)
    refused('sttode_pmath_hsoftmax_bwd_c', 'gc_ws', one, one, one, one, one, one, one, one, 4, 4, 4, one, one, None, None)


def test_fixture_holds_the_cases_and_the_reference_handles_them(golden):
    zc = golden('pmath_cgrad')
    cs = cases(zc, golden('pmath_vjp'), golden('pmath_vjp_rows'))
    names = {c['name'] for c in cs}
    assert len([n for n in names if n.startswith('row.')]) == len(ROW_OPS) * len(ROW_SHAPES) == 240 and zc['row.gc'].shape == (2, 12, 20)
    for n in ('clip.project.c1.0', 'clip.project.c0.5', 'zero.expmap0', 'zero.logmap0', 'zero.expmap', 'bcast.mobius_add', 'bcast.dist'):
        assert n in names, n
    assert all('mv.' + t in names for t in MATVEC) and all('dm.P%dR%dd%d' % s in names for s in DIST_MATRIX)
    assert all('edge.%s.n%d' % (op, n) in names for op in EDGE_OPS for n in EDGE_ROWS) and zc['edge.in'].shape == (3, 1030, 5)
    assert all(p + 'B%dC%dd%d' % s in names for p in ('hs.', 'mab.') for s in PAIR_SHAPES)
    r = np.sqrt(2.0) * np.linalg.norm(zc['edge.in'][:2], axis=-1)              # the domain: sqrt(c) |.| in [0.05, 0.9]
    assert (r > 0.0499).all() and (r < 0.9001).all()
    worst = {}
    for c in cs:
        assert np.isfinite(c['gc64']), c['name']
        e = err(c['gc32'], c['gc64'])
        worst[c['op']] = max(worst.get(c['op'], 0.0), e)
        assert e <= BOUND, (c['name'], e)
    for name, (params, ins) in MODULES.items():
        for k in params + ins + ('c',):
            g = zc['%s.g%s' % (name, k)]
            assert g.shape[0] == 2 and np.isfinite(g).all() and (k == 'c') == (g.shape == (2, 1)), (name, k, g.shape)
            if k not in ('c',) + ins:
                assert g.shape[1:] == zc['%s.%s' % (name, k)].shape
            e = err(g[1], g[0])
            worst[name] = max(worst.get(name, 0.0), e)
            assert e <= BOUND, (name, k, e)
        assert np.abs(zc[name + '.gc'][0]).max() > 1e-3, name + ': a c gradient this small checks nothing'
    print('reference fp32 against its float64, worst per op: ' + ', '.join('%s %.1e' % kv for kv in sorted(worst.items())))
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    assert os.path.getsize(os.path.join(here, 'pmath_cgrad.npz')) < 300 * 1000
