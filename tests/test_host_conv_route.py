"""The host dispatch of the sparse conv and linear layers (functional._conv_route / _dense_route) against the rule it replaced,
on a grid of shapes; no GPU, but the built library (its *_supported queries), as tests/test_cabi_symbols.py.

THE OLD RULE is restated here as plain functions over the library's queries: the bodies, as they were before the route record,
of _conv_os's ladder, _lk_route, _rows16_volume_ok, _conv_rows16_ok, conv_epilogue_supported, TileSchedule.run's and
PairSchedule.run's choice of entry and _dense_x3_ok / _dense_x3's.  They read the environment switches where the old code read
them, so the comparison holds under any setting; the switches themselves are exercised in child processes (functional.py
reads U2MKD_PAIRS_X3 and U2MKD_LINEAR_X3 at import)."""
import itertools
import os
import subprocess
import sys

import torch

import conv_fwd_f64_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
TAG = {BF16: '_bf16', F16: '_f16'}
ROWS = (F32, BF16, F16)
CHANNELS = (4, 16, 32, 48, 64, 96, 128, 136, 192, 256, 512)
VOLUMES = (1, 8, 27, 31, 32, 64, 65, 125, 343)
N_ROWS = (800, 23999, 24000, 80000)          # 24 000: the threshold of _pairs_mode at cin * cout = 8192
SWITCHES = ('U2MKD_CONV_SCHEDULE', 'U2MKD_PAIRS_X3', 'U2MKD_LINEAR_X3', 'U2MKD_CONV_ARITH')


def _lib():
    from u2mkd_amd import _lib
    return _lib.load()


def _functional():
    from u2mkd_amd.torchsparse.nn import functional
    return functional


# ---- the rule before the route record ------------------------------------------------------------------------------------------

def _on(name):
    return os.environ.get(name, '1') != '0'


def old_pairs_mode(cin, cout, n_rows=0):
    env = os.environ.get('U2MKD_CONV_SCHEDULE')
    if env in ('tiles', 'pairs'):
        return env == 'pairs'
    if cout % 4:
        return False
    return cin * cout > 8192 or (cin * cout == 8192 and n_rows < 24000)


def old_lk_route(cin, cout, k, n_rows, rows16=False):
    return k > 64 or (k > 31 and not rows16 and not old_pairs_mode(cin, cout, n_rows))


def old_conv_rows16_ok(cin, cout):
    return cin >= 32 and cin % 32 == 0 and cout >= 32 and cout % 32 == 0


def old_rows16_volume_ok(lib, cin, cout, k):
    if k <= 31:
        return True
    return k <= 64 and not lib.u2mkd_conv_tiles_supported(cin, cout, k)


def old_epilogue_supported(lib, rows, cin, cout, k, n_rows):
    """conv_epilogue_supported without the autocast state: fp32 rows, multiples of 4"""
    if rows != F32 or cin % 4 or cout % 4:
        return False
    if old_lk_route(cin, cout, k, n_rows):
        return False
    if old_pairs_mode(cin, cout, n_rows):
        return True
    return bool(lib.u2mkd_conv_tiles_supported(cin, cout, k)) and os.environ.get('U2MKD_CONV_SCHEDULE') in (None, 'tiles', 'pairs')


LK = ('lk', 'u2mkd_conv_forward_lk', None, 0, False)


def old_conv_os(lib, rows, cin, cout, k, n_rows, epilogue):
    """(schedule, product entry, gather-sum entry, arith of the weights, fragment order) of _conv_os, TileSchedule.run and
    PairSchedule.run as they were; ``epilogue`` only where old_epilogue_supported holds (nothing else was ever passed one)"""
    if k > 64:
        return LK
    rows16 = rows != F32
    if rows16 and not lib.u2mkd_conv_tiles_supported(cin, cout, k):
        return 'pairs', 'u2mkd_conv_forward_pairs' + TAG[rows], 'u2mkd_pairs_gather_sum' + TAG[rows], 5 if rows == F16 else 3, True
    if not rows16 and old_pairs_mode(cin, cout, n_rows):
        x3 = _on('U2MKD_PAIRS_X3') and bool(lib.u2mkd_conv_pairs_x3_supported(cin, cout))
        f2 = x3 and bool(lib.u2mkd_conv_pairs_f16x2_supported(cin, cout))
        entry = 'u2mkd_conv_forward_pairs' + ('_f16x2' if f2 else ('_x3' if x3 else ''))
        return 'pairs', entry, 'u2mkd_pairs_gather_sum_ep' if epilogue else 'u2mkd_pairs_gather_sum', 4 if f2 else 0, bool(x3)
    if k > 31:
        return LK
    ar = 4 if not rows16 and lib.u2mkd_conv_tiles_arith(cin, cout, k) == 4 else 0
    if epilogue:
        return 'tiles', 'u2mkd_conv_forward_tiles_ep', None, ar, True
    if rows16:
        return 'tiles', 'u2mkd_conv_forward_tiles' + TAG[rows], None, 5 if rows == F16 else 3, True
    if lib.u2mkd_conv_tiles_supported(cin, cout, k):
        return 'tiles', 'u2mkd_conv_forward_tiles', None, ar, True
    return 'tiles', 'u2mkd_conv_forward_sorted', None, 0, False


def old_dense(lib, rows, cin, cout):
    """(entry, arith, fragment order) of LinearFunction's choice (ctx.x3) and _dense_x3's / _dense's launch"""
    if rows != F32:
        return 'u2mkd_linear_forward' + TAG[rows], 5 if rows == F16 else 3, True
    if _on('U2MKD_PAIRS_X3') and _on('U2MKD_LINEAR_X3') and bool(lib.u2mkd_conv_pairs_x3_supported(cin, cout)):
        f2 = bool(lib.u2mkd_conv_pairs_f16x2_supported(cin, cout))
        return ('u2mkd_linear_forward_f16x2' if f2 else 'u2mkd_linear_forward_x3'), 4 if f2 else 0, True
    return 'u2mkd_linear_forward', 0, False


# ---- the checks (also run in child processes: ``python test_host_conv_route.py rule | family``) -----------------------------------

def grid():
    return itertools.product(ROWS, CHANNELS, CHANNELS, VOLUMES, N_ROWS)


def rule_mismatches():
    """every grid point where _conv_route / _dense_route differ from the old rule, and the number of points compared"""
    F, lib = _functional(), _lib()
    bad, n = [], 0
    for rows, cin, cout, k, n_rows in grid():
        can_fold = old_epilogue_supported(lib, rows, cin, cout, k, n_rows)
        for ep in (False, True):
            r = F._conv_route(rows, cin, cout, k, n_rows, epilogue=ep)
            n += 1
            if r.epilogue != can_fold:
                bad.append(('epilogue', rows, cin, cout, k, n_rows, ep, r))
            if ep and not can_fold:
                continue                # (the old code never launched this; the new _conv_os raises on it)
            if (r.schedule, r.entry, r.gather, r.arith, r.fragments) != old_conv_os(lib, rows, cin, cout, k, n_rows, ep):
                bad.append(('conv', rows, cin, cout, k, n_rows, ep, r))
    for rows, cin, cout in itertools.product(ROWS, CHANNELS, CHANNELS):
        r = F._dense_route(rows, cin, cout)
        n += 1
        entry, arith, fragments = old_dense(lib, rows, cin, cout)
        if (r.schedule, r.entry, r.gather, r.arith, r.fragments, r.epilogue) != ('dense', entry, None, arith, fragments, False):
            bad.append(('dense', rows, cin, cout, r))
    return bad, n


def family_mismatches():
    """default settings, k <= 31: the route's entry against conv_fwd_f64_ref.family; where family has no 16-bit kernel the layer
    must stay on fp32 rows and run family's fp32 entry"""
    F = _functional()
    bad, n = [], 0
    for rows, cin, cout, k, n_rows in grid():
        if k > 31:
            continue
        n += 1
        try:
            want = R.family(cin, cout, rows, n_rows, k)[0]
            got = F._conv_route(rows, cin, cout, k, n_rows).entry
        except ValueError:
            if F._rows16_servable(rows, cin, cout, k):
                bad.append(('16-bit rows without a kernel', rows, cin, cout, k))
            want = R.family(cin, cout, F32, n_rows, k)[0]
            got = F._conv_route(F32, cin, cout, k, n_rows).entry
        if got != want:
            bad.append((rows, cin, cout, k, n_rows, got, want))
    return bad, n


def _child(what, env):
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    code = 'import sys; sys.path[:0] = [%r, %r]\nimport test_host_conv_route as T\nbad, n = T.%s_mismatches()\nprint("compared", n, "bad", len(bad), bad[:5])' \
           % (ROOT, os.path.join(ROOT, 'tests'), what)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300, env=dict(base, **env))
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.split()


# ---- the tests -----------------------------------------------------------------------------------------------------------------

def test_routes_equal_the_rule_they_replace():
    bad, n = rule_mismatches()
    assert n == 2 * 3 * 11 * 11 * 9 * 4 + 3 * 11 * 11
    assert not bad, (len(bad), bad[:5])


def test_route_entries_equal_the_family_the_float64_tests_predict():
    out = _child('family', {})
    assert out[:4] == ['compared', str(3 * 11 * 11 * 4 * 4), 'bad', '0'], out


def test_sixteen_bit_rows_are_chosen_only_where_both_launches_take_them():
    """the forward is cin -> cout over the map's outputs, the input gradient cout -> cin over its inputs, on the same rows; and the
    choice is the old one (_conv_rows16_ok and _rows16_volume_ok) on every shape"""
    F, lib = _functional(), _lib()
    chosen = 0
    for rows, cin, cout, k in itertools.product((BF16, F16), CHANNELS, CHANNELS, VOLUMES):
        ok = F._rows16_servable(rows, cin, cout, k)
        assert ok == bool(old_conv_rows16_ok(cin, cout) and old_rows16_volume_ok(lib, cin, cout, k)), (rows, cin, cout, k)
        if not ok:
            continue
        chosen += 1
        for n_rows in N_ROWS:
            for ca, cb in ((cin, cout), (cout, cin)):
                r = F._conv_route(rows, ca, cb, k, n_rows)
                assert r.schedule in ('tiles', 'pairs') and r.entry.endswith(TAG[rows]), (rows, ca, cb, k, n_rows, r)
                assert r.arith == F._arith16(rows) and r.fragments
                if r.schedule == 'tiles':
                    assert lib.u2mkd_conv_tiles_supported(ca, cb, k) and k <= 31
                else:
                    assert r.gather == 'u2mkd_pairs_gather_sum' + TAG[rows] and lib.u2mkd_conv_pairs_x3_supported(ca, cb)
    assert chosen


def test_one_arith_code_and_one_fragment_slot_per_entry():
    """Every entry of the table reads weights of exactly ONE arith code -- but for the two fp32-row tile entries, which take the
    code as an argument of the call (the library default or f16x2): they are pinned to exactly those two codes."""
    F = _functional()
    table = F._ENTRY_WEIGHTS
    one = {'u2mkd_conv_forward_pairs_x3': 0, 'u2mkd_conv_forward_pairs_f16x2': 4, 'u2mkd_conv_forward_pairs_bf16': 3,
           'u2mkd_conv_forward_pairs_f16': 5, 'u2mkd_conv_forward_tiles_bf16': 3, 'u2mkd_conv_forward_tiles_f16': 5,
           'u2mkd_linear_forward': 0, 'u2mkd_linear_forward_x3': 0, 'u2mkd_linear_forward_f16x2': 4, 'u2mkd_linear_forward_bf16': 3,
           'u2mkd_linear_forward_f16': 5, 'u2mkd_conv_forward_pairs': 0, 'u2mkd_conv_forward_sorted': 0, 'u2mkd_conv_forward_lk': 0}
    for entry, arith in one.items():
        assert table[entry][0] == (arith,), entry
    # the fp32-row tile entries take the code as an ARGUMENT: the library default or f16x2, nothing else
    by_argument = {e for e in table if e not in one}
    assert by_argument == {'u2mkd_conv_forward_tiles', 'u2mkd_conv_forward_tiles_ep'}
    assert all(table[e] == ((0, 4), True) for e in by_argument)
    # fragment order exactly where the weights are not the plain fp32 tensor; 16-bit entries on their own plane
    for entry, (codes, fragments) in table.items():
        assert fragments == (entry not in ('u2mkd_conv_forward_lk', 'u2mkd_conv_forward_sorted', 'u2mkd_conv_forward_pairs',
                                           'u2mkd_linear_forward')), entry
        for dt in (BF16, F16):
            assert entry.endswith(TAG[dt]) == (codes == (F._arith16(dt),)), entry
    # one cache slot per code, one code per slot
    slots = F._WFRAG_SLOT
    assert set(slots) == {c for codes, _ in table.values() for c in codes} == {0, 3, 4, 5}
    assert len(set(slots.values())) == len(slots)
    # every route names an entry of the table, with a code the entry takes and the slot of that code
    for rows, cin, cout, k, n_rows in grid():
        for r in (F._conv_route(rows, cin, cout, k, n_rows), F._conv_route(rows, cin, cout, k, n_rows, True), F._dense_route(rows, cin, cout)):
            assert r.arith in table[r.entry][0] and r.fragments == table[r.entry][1] and r.arith in slots, r


def test_environment_switches_move_the_route_as_they_moved_the_rule():
    """U2MKD_CONV_SCHEDULE = tiles / pairs and U2MKD_PAIRS_X3 = 0, each in a process of its own"""
    total = str(2 * 3 * 11 * 11 * 9 * 4 + 3 * 11 * 11)
    for env in ({'U2MKD_CONV_SCHEDULE': 'tiles'}, {'U2MKD_CONV_SCHEDULE': 'pairs'}, {'U2MKD_PAIRS_X3': '0'}, {'U2MKD_LINEAR_X3': '0'}):
        out = _child('rule', env)
        assert out[:4] == ['compared', total, 'bad', '0'], (env, out)
