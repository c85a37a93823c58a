"""Generator of tests/golden/sptr_pos_embedding.npz: outputs of the REFERENCE's position embedding class
(third_party/SparseTransformer/sptr/position_embedding.py, imported from the reference checkout at generation time only;
the file itself needs nothing but torch) on two small scenes, for tests/test_sptr_module.py.

    python tests/golden/make_sptr_pe_golden.py [reference checkout, default /root/reference]

Stored: the points of the two scenes (``xyz0`` [40, 3], ``xyz1`` [25, 3], fp32), and per (pos_type, d_pos) in
{sine, fourier} x {32, 48} with normalize=True: ``<type>_<d>_scene<i>`` [points, d_pos] -- the embedding over the scene's own
bounding box, transposed the way sptr/modules.py:140-142 uses it -- and for fourier ``fourier_<d>_gauss_B`` [3, d / 2], the
class's random matrix, as data."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def main(ref):
    path = os.path.join(ref, 'third_party', 'SparseTransformer', 'sptr', 'position_embedding.py')
    spec = importlib.util.spec_from_file_location('reference_position_embedding', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    g = torch.Generator().manual_seed(20)
    scenes = [torch.rand(40, 3, generator=g) * torch.tensor([50.0, 40.0, 4.0]) - torch.tensor([25.0, 20.0, 3.0]),
              torch.rand(25, 3, generator=g) * torch.tensor([8.0, 70.0, 2.5]) + torch.tensor([3.0, -35.0, -1.0])]
    out = {'xyz0': scenes[0].numpy(), 'xyz1': scenes[1].numpy()}
    for pos_type in ('sine', 'fourier'):
        for d in (32, 48):
            torch.manual_seed(100 + d)
            pe = mod.PositionEmbeddingCoordsSine(pos_type=pos_type, d_pos=d, normalize=True)
            if pos_type == 'fourier':
                out[f'fourier_{d}_gauss_B'] = pe.gauss_B.numpy().copy()
            for i, p in enumerate(scenes):
                e = pe(p[None].clone(), input_range=[p.min(0)[0][None], p.max(0)[0][None]])
                out[f'{pos_type}_{d}_scene{i}'] = e[0].permute(1, 0).contiguous().numpy()
    dst = os.path.join(HERE, 'sptr_pos_embedding.npz')
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), 'bytes', sorted(out))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else '/root/reference')
