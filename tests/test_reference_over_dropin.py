"""The reference's model call sequence imports and constructs over the HIP drop-in (``install_as_torchsparse()`` /
``install_as_sptr()``).  Construct-only (parameters live on the CPU; every operator of the drop-in refuses CPU tensors).
The reference's own model files are not part of this repository, so the call sequence is the oracle's line-by-line
restatement of them (oracle/spvcnn_ref.py, oracle/spformer_ref.py: pinned bit for bit against the reference's classes by
tests/test_golden_*.py), re-bound to the installed ``torchsparse`` / ``sptr`` names with ``over()``.  What is checked is
that the package surface is complete enough for that sequence and that the models come out with what the reference's
own SPVCNN / SPVCNN_SPFORMER classes gave over the same drop-in when the fixtures were recorded: the parameter counts
(5 449 169 / 21 777 809 / 87 073 553 for cr 0.5 / 1.0 / 2.0; 23 033 729 for SPVCNN_SPFORMER cr 1.0 with
its 4 SphereFormer blocks) and the state-dict names and shapes of tests/golden/{spvcnn_cr05,spformer_cr10}_keys.json."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, 'tests', 'golden')

CHILD = r'''
import json, sys
sys.path.insert(0, %(root)r)
import numpy as np
import u2mkd_amd
u2mkd_amd.install_as_torchsparse()
u2mkd_amd.install_as_sptr()

import torchsparse, torchsparse.nn as spnn
import third_party.SparseTransformer.sptr as sptr
assert torchsparse.__name__ == 'u2mkd_amd.torchsparse'
assert sptr.__name__ == 'u2mkd_amd.sptr'
from oracle import spformer_ref, spvcnn_ref
SV = spvcnn_ref.over(torchsparse)
SF = spformer_ref.over(torchsparse, sptr)
assert SF.sptr is sptr
shapes = lambda m: {k: list(v.shape) for k, v in m.state_dict().items()}
counts = {}
for cr in (0.5, 1.0, 2.0):
    m = SV.SPVCNN(cr=cr, in_channel=4, num_classes=17, pres=0.05, vres=0.05)
    counts[cr] = sum(p.numel() for p in m.parameters())
    convs = [x for x in m.modules() if isinstance(x, spnn.Conv3d)]
    assert len(convs) == 49, len(convs)
    assert all(c.kernel.dim() in (2, 3) for c in convs)
    if cr == 0.5:
        print('SPVCNN_SHAPES', json.dumps(shapes(m)))
print('COUNTS', counts[0.5], counts[1.0], counts[2.0])

kw = dict(pres=0.05, vres=0.05, window_size=np.array([0.3, 0.3, 0.3]),
          window_size_sphere=[2, 2, 120], quant_size=np.array([0.3, 0.3, 0.3]) / 24, quant_size_sphere=np.array([2, 2, 120]) / 24,
          window_size_scale=[2.0, 2.0], drop_path_rate=0.3, a=0.05 * 0.25)
t = SF.SPVCNN_SPFORMER(cr=1.0, in_channel=4, num_classes=17, **kw)
blocks = [x for x in t.modules() if isinstance(x, SF.SphereFormer)]
print('SPFORMER', len(blocks), sum(p.numel() for p in t.parameters()))
print('SPFORMER_SHAPES', json.dumps(shapes(t)))
'''


def test_reference_call_sequence_constructs_over_the_dropin():
    r = subprocess.run([sys.executable, '-c', CHILD % {'root': ROOT}], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = dict(line.split(' ', 1) for line in r.stdout.strip().splitlines() if ' ' in line)
    assert out['COUNTS'].split() == ['5449169', '21777809', '87073553'], out['COUNTS']
    n_blocks, n_params = (int(v) for v in out['SPFORMER'].split())
    assert n_blocks == 4 and n_params == 23033729
    for key, fixture in (('SPVCNN_SHAPES', 'spvcnn_cr05_keys.json'), ('SPFORMER_SHAPES', 'spformer_cr10_keys.json')):
        with open(os.path.join(G, fixture)) as f:
            assert json.loads(out[key]) == json.load(f), fixture
