"""Synthetic neighbour tables for the large-kernel-volume convolution (csrc/conv_lk.hip: u2mkd_conv_forward_lk walks the offsets
in chunks of 32), the cases tests/test_gpu_conv_lk_f64.py and tests/test_gpu_conv_lk_wgrad.py run on them, and the wrong
evaluations tests/test_host_conv_lk_bound.py holds the bound against (test helper; plain torch, CPU tensors).

The reference, the roles, the rows, the weights and the bound are those of tests/conv_fwd_f64_ref.py; only the tables are new,
because its patterns stop at 27 offsets.  EVERY OFFSET'S MAP IS INJECTIVE, as in a real kernel map.  ``TABLES`` names
(K, n_in, n_out, placement):

    K          32 (one full chunk), 33 (a chunk of one offset), 63, 64 (two full chunks), 65, 125 (k = 5), 129 and 343 (k = 7)
    n_out      1, 63, 64, 65 and 129 (conv_fwd_f64_ref.TAILS: the 64-row tile and its tails)
    placement  'dense'      every offset holds pairs; about an eighth of the rows have no neighbour at any offset
               'last'       the only live offsets are in the LAST chunk: the chunks before it cost an index burst and nothing else
                            (K = 63: offsets 32 .. 62, so that offset 32 is still there to be dropped by a degraded form)
               'gap'        an entirely empty MIDDLE chunk (offsets 64 .. 95), live chunks on both sides of it
               'deadblock'  the 16-row block of rows 16 .. 31 has no neighbour at any offset (its wave skips every product by
                            ballot); the other blocks are dense
    n_in != n_out in the tables 'ns65' and 'ns125': the inverse roles walk ``invert(nbr, n_in)``, derived here from nbr alone.

``CASES`` pairs every table with roles, launch widths (cin in {4, 20, 32, 96}: 20 is already a multiple of 4, so it is passed
as it is; cout in {4, 24, 32, 48, 96}: 24 and 48 leave a partly filled 16-column block) and a spread of make_rows, so that
every K, every n_out, every placement, every role, every width and every spread is run at least once; the widest products sit
on the smaller volumes, which keeps a case's float64 and fp32 references at a second or two."""
import torch

import conv_fwd_f64_ref as R

CHUNK = 32

# name -> (K, n_in, n_out, placement)
TABLES = {
    't32': (32, 64, 64, 'dense'),
    't33': (33, 65, 65, 'dense'),
    't63': (63, 63, 63, 'last'),
    't64': (64, 129, 129, 'deadblock'),
    't65': (65, 1, 1, 'dense'),
    't125': (125, 129, 129, 'gap'),
    't129': (129, 65, 65, 'dense'),
    't343': (343, 64, 64, 'gap'),
    'ns65': (65, 150, 63, 'dense'),
    'ns125': (125, 100, 129, 'deadblock'),
}
# tables of tests/test_gpu_conv_lk_wgrad.py alone: K = 128 is two full weight-gradient blocks of 64 offsets
WGRAD_TABLES = {'t128': (128, 100, 129, 'dense')}
# (table, cin, cout) of the weight-gradient cases: K = 64 (one block), 65 (a block of one offset), 128, 129 and 343 (six blocks)
WGRAD_CASES = [(t, ci, co) for t in ('t64', 'ns65', 't128', 't129', 't343') for ci, co in ((4, 32), (32, 32), (64, 64))]
WGRAD_BLOCK = 64
SQUARE = tuple(n for n, t in TABLES.items() if t[1] == t[2])

# (table, role, cin, cout, spread) of every launch the GPU test makes and the host test evaluates
CASES = [
    ('t32', 'fwd', 32, 32, 'rows'), ('t32', 'flip', 4, 48, 'unit'),
    ('t33', 'fwd', 20, 24, 'rows'), ('t33', 'flip', 32, 32, 'tiny'),
    ('t63', 'fwd', 96, 4, 'unit'), ('t63', 'flip', 20, 96, 'rows'),
    ('t64', 'fwd', 4, 32, 'rows'), ('t64', 'flip', 32, 24, 'rows'),
    ('t65', 'fwd', 32, 48, 'rows'), ('t65', 'flip', 4, 4, 'unit'),
    ('t125', 'fwd', 4, 32, 'rows'), ('t125', 'flip', 32, 32, 'rows'), ('t125', 'fwd', 96, 96, 'unit'),
    ('t129', 'fwd', 20, 48, 'rows'), ('t129', 'flip', 32, 4, 'rows'),
    ('t343', 'fwd', 4, 24, 'rows'), ('t343', 'flip', 20, 32, 'unit'), ('t343', 'fwd', 32, 32, 'tiny'),
    ('ns65', 'fwd', 32, 24, 'rows'), ('ns65', 'inv', 32, 32, 'rows'), ('ns65', 'invT', 4, 96, 'unit'), ('ns65', 'fwdT', 96, 24, 'rows'),
    ('ns125', 'fwd', 20, 32, 'unit'), ('ns125', 'inv', 96, 32, 'rows'), ('ns125', 'invT', 32, 48, 'rows'), ('ns125', 'fwdT', 20, 32, 'tiny'),
]
# (r is a maximum over the elements of a case: on the 100 x 4 outputs of 'ns125' 'inv' 32 -> 4 it was too poor a sample -- the
# second honest order came to 0.81 of the bound, which tests/test_host_conv_lk_bound.py does not accept of a case -- so that role
# runs 96 -> 32 there and the 4-column launches are on t63, t65 and t129.)
# (the launch widths of the transposed roles: ca = the kernel's cout, cb = its cin -- 'fwdT' 96 -> 24 is the input gradient of a
# transposed 24 -> 96 layer)


def n_chunks(k_total):
    return -(-k_total // CHUNK)


def make_table(name):
    """(nbr int32 [K, n_out], n_in) of a named table; the same on every machine"""
    k_total, n_in, n_out, placement = TABLES[name] if name in TABLES else WGRAD_TABLES[name]
    g = torch.Generator().manual_seed(611953 * k_total + 8191 * n_out + n_in)
    nbr = torch.full((k_total, n_out), -1, dtype=torch.int64)
    rows_alive = torch.rand(n_out, generator=g) >= 0.125            # rows without a neighbour at any offset
    rows_alive[:2] = True
    if n_out > 3:
        rows_alive[n_out - 2] = False                               # (at least one, and in the tile's tail)
    if placement == 'deadblock':
        rows_alive[16:32] = False
    last = n_chunks(k_total) - 1
    # THE LAST LIVE PAIR of the table is (offset K - 1, output row 0, input row 0), the only pair of that offset, of that output
    # row and of that input row: a walk that skips it turns a whole row into zeros, whatever the other rows weigh (make_rows keeps
    # row 0 a full row).  A table of one row has nothing else to give.
    lone = n_out > 1
    for k in range(k_total - 1 if lone else k_total):
        chunk = k // CHUNK
        if placement == 'last' and chunk != last:
            continue
        if placement == 'gap' and chunk == 2:
            continue
        has = (torch.rand(n_out, generator=g) < 0.4) & rows_alive
        if k in (CHUNK, k_total - 1, CHUNK * last):                 # offset 32, the last offset and the last chunk's first: never empty
            has[1 if lone else 0] = True
        if lone:
            has[0] = False
        rows = torch.nonzero(has)[:, 0]
        rows = rows[torch.randperm(len(rows), generator=g)][:n_in - lone]   # injective: no input row twice in an offset
        nbr[k, rows] = torch.randperm(n_in - lone, generator=g)[:len(rows)] + int(lone)
    if lone:
        nbr[k_total - 1, 0] = 0
    assert int(nbr.max()) < n_in and int(nbr.min()) >= -1
    return nbr.int().contiguous(), n_in


def invert(nbr, n_in):
    """nbr_inv int32 [K, n_in]: the output row fed by input row i through offset k (-1: none), from ``nbr`` alone"""
    k_total, n_out = nbr.shape
    inv = torch.full((k_total, n_in), -1, dtype=torch.int32)
    for k in range(k_total):
        j = torch.nonzero(nbr[k] >= 0)[:, 0]
        inv[k, nbr[k][j].long()] = j.int()
    return inv.contiguous()


def rulebook(nbr):
    """torchsparse's (nbmaps int32 [P, 2] rows (in, out) grouped by offset with ascending out index, nbsizes [K]) of a table"""
    kk, jj = torch.nonzero(nbr >= 0, as_tuple=True)                 # row-major: by k, then j
    return torch.stack([nbr[kk, jj].long(), jj], dim=1).int().contiguous(), (nbr >= 0).sum(dim=1).int()


def make_wgrad_case(case):
    """CPU tensors of a weight-gradient case: rows x [n_in, cin] and output gradients g [n_out, cout], every row its own power of
    ten (1e-10 .. 1e10, as tests/wgrad_f64_ref.py's 'rows' spread), a tenth of the rows zero; the kernel w [K, cin, cout]"""
    name, cin, cout = case
    nbr, n_in = make_table(name)
    k_total, n_out = nbr.shape
    g = torch.Generator().manual_seed(1299709 * k_total + 31 * cin + cout)
    x, dy = torch.randn(n_in, cin, generator=g), torch.randn(n_out, cout, generator=g)
    x = x * torch.pow(10.0, torch.randint(-10, 11, (n_in, 1), generator=g).float())
    dy = dy * torch.pow(10.0, torch.randint(-10, 11, (n_out, 1), generator=g).float())
    x[torch.rand(n_in, generator=g) < 0.1] = 0.0
    dy[torch.rand(n_out, generator=g) < 0.1] = 0.0
    return {'nbr': nbr, 'n_in': n_in, 'x': x, 'dy': dy, 'w': R.make_weights(k_total, cin, cout), 'k': k_total}


def make_case(case):
    """CPU tensors of one case: conv_fwd_f64_ref.make_case's dictionary on a table of this module"""
    name, role, ca, cb, spread = case
    nbr, n_in = make_table(name)
    k_total = nbr.shape[0]
    seed = sorted(TABLES).index(name)
    n_src = n_in if role in R.ON_OUTPUTS else nbr.shape[1]
    w = R.make_weights(k_total, cb if role in R.TRANSPOSED else ca, ca if role in R.TRANSPOSED else cb, spread, seed)
    return {'nbr': nbr, 'n_in': n_in, 'x': R.make_rows(spread, n_src, ca, torch.float32, seed), 'w': w, 'role': role, 'k': k_total}


def launch(c):
    """What u2mkd_conv_forward_lk takes for a case: (table [K, n_rows], weights [K, cb, ca] row-major with the reduction
    contiguous, kflip).  'fwd' / 'invT' multiply by w[k] (transposed into that layout), 'flip' / 'inv' / 'fwdT' by w[k]^T (the
    tensor as it is); the inverse roles walk the inverse table."""
    role = c['role']
    tbl = c['nbr'] if role in R.ON_OUTPUTS else invert(c['nbr'], c['n_in'])
    wt = (c['w'] if role in R.TRANSPOSED else c['w'].transpose(1, 2)).contiguous()
    return tbl, wt, int(role == 'flip')


# ---- wrong evaluations of a chunked walk -------------------------------------------------------------------------------------

def _matrix(c, kw):
    w = c['w'].float()
    return w[kw].t() if c['role'] in R.TRANSPOSED else w[kw]


def _weight_index(c, k):
    return c['k'] - 1 - k if c['role'] == 'flip' else k


def _honest(c, nbr=None, **kw):
    return R.honest_fp32(c['x'], c['w'], c['nbr'] if nbr is None else nbr, c['n_in'], c['role'], running=True, **kw)


def _last_chunk_dropped(c):
    nbr = c['nbr'].clone()
    nbr[CHUNK * (n_chunks(c['k']) - 1):] = -1
    return _honest(c, nbr)


def _flip_inside_chunks(c):
    def mat(k):
        c0 = k - k % CHUNK
        size = min(CHUNK, c['k'] - c0)
        return _matrix(c, c0 + size - 1 - (k - c0))
    return _honest(c, mat=mat)


def _weights_of_previous_chunk(c):
    return _honest(c, mat=lambda k: _matrix(c, _weight_index(c, k - CHUNK if k >= CHUNK else k)))


def _last_live_pair_skipped(c):
    nbr = c['nbr'].clone()
    k = int(torch.nonzero((nbr >= 0).any(dim=1))[-1])
    nbr[k, int(torch.nonzero(nbr[k] >= 0)[-1])] = -1
    return _honest(c, nbr)


# name -> (applies to the case?, f(case) -> fp32 result)
DEGRADED = {
    'the last chunk dropped': (lambda c: True, _last_chunk_dropped),
    'offset 32 dropped': (lambda c: c['k'] > CHUNK, lambda c: _honest(c, skip=CHUNK)),
    # (K = 32: one chunk, mirroring inside it IS mirroring over the volume, and there is no chunk before it)
    'kflip mirrored inside each chunk': (lambda c: c['role'] == 'flip' and c['k'] > CHUNK, _flip_inside_chunks),
    'the weights of chunk c taken from chunk c - 1': (lambda c: c['k'] > CHUNK, _weights_of_previous_chunk),
    # (the tables make that pair the only one of its rows, see make_table: visible on every case)
    'the last live pair skipped': (lambda c: True, _last_live_pair_skipped),
}
