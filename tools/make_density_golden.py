"""Writes tests/golden/density_orient.npz: inputs and the image the REFERENCE's draw_orient_density returns for them.

    python tools/make_density_golden.py [--reference DIR] [--out FILE]

The reference's function (EPro-PnP-6DoF lib/utils/draw_orient_density.py) is imported from the reference checkout at run time --
nothing of it is stored here -- with a stub module `cv2` whose `line` does nothing in sys.modules (cv2 is not installed; the lines
are the one part of the picture the package does not reproduce pixel for pixel, so the fixture is the picture without them).
Runs on the CPU.  Two cases:
    a  (S,B,size) = (32,2,64), the reference's defaults
    b  (96,3,64), sample_kernel=(3,3), saturation=0.7, sphere_opacity=0.4, intensity_scale=20
Inputs: a random base quaternion per object plus 0.3 x noise, normalised; log-weights 2 x normal.  A case is fenced from fp64: no
axis point within 1e-4 px of a pixel boundary and none with |a_z| < 1e-5, so that an fp32 implementation takes the reference's
binning decisions whatever its rounding.  Seeds are tried from the case's first seed upwards; the first that passes is taken (the
same one on every run: the file regenerates bit for bit).
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('EPROPNP_REFERENCE', '/root/reference')
OUT = os.path.join(ROOT, 'tests', 'golden', 'density_orient.npz')
CASES = {
    'a': dict(S=32, B=2, size=64, seed=100, kwargs={}),
    'b': dict(S=96, B=3, size=64, seed=200, kwargs=dict(sample_kernel=(3, 3), saturation=0.7, sphere_opacity=0.4, intensity_scale=20)),
}
FENCE_PX, FENCE_Z = 1e-4, 1e-5


def reference_function(ref=REF):
    path = os.path.join(ref, 'EPro-PnP-6DoF', 'lib', 'utils', 'draw_orient_density.py')
    stub = types.ModuleType('cv2')
    stub.line = lambda *a, **k: None
    saved = sys.modules.get('cv2')
    sys.modules['cv2'] = stub
    try:
        spec = importlib.util.spec_from_file_location('reference_draw_orient_density', path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        if saved is None:
            del sys.modules['cv2']
        else:
            sys.modules['cv2'] = saved
    return mod.draw_orient_density


def inputs(S, B, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(1, B, 4, generator=g) + 0.3 * torch.randn(S + 1, B, 4, generator=g)
    q = q / q.norm(dim=-1, keepdim=True)
    pose = torch.cat((torch.randn(S + 1, B, 3, generator=g), q), -1)
    logw = 2.0 * torch.randn(S, B, generator=g)
    return pose[0].contiguous(), pose[1:].contiguous(), logw.contiguous()


def fenced(pose_samples, size):
    """no axis point within FENCE_PX of a pixel boundary, none with |a_z| < FENCE_Z (fp64)"""
    q = pose_samples[..., 3:].double().numpy()
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    dd = w * w - (x * x + y * y + z * z)
    ax = np.stack((2 * x * x + dd, 2 * (x * y - w * z), 2 * (x * z + w * y)), -1)
    ay = np.stack((2 * (x * y + w * z), 2 * y * y + dd, 2 * (y * z - w * x)), -1)
    az = np.stack((2 * (x * z - w * y), 2 * (y * z + w * x), 2 * z * z + dd), -1)
    f = np.stack((ax, ay)) * (0.4 * size) + (size / 2 - 0.5)
    boundary = np.abs(f - np.floor(f) - 0.5)
    return float(boundary.min()) > FENCE_PX and float(np.abs(az).min()) > FENCE_Z


def make(ref=REF):
    fn = reference_function(ref)
    out = {}
    for name, c in CASES.items():
        for seed in range(c['seed'], c['seed'] + 16):
            pose_opt, pose_samples, logw = inputs(c['S'], c['B'], seed)
            if fenced(pose_samples, c['size']):
                break
        else:
            raise AssertionError(f'case {name}: no fenced seed among 16')
        assert fenced(pose_samples, c['size'])
        with torch.no_grad():
            image = fn(pose_opt, pose_samples, logw, size=c['size'], **c['kwargs'])
        out[f'{name}_seed'] = np.int64(seed)
        out[f'{name}_pose_opt'] = pose_opt.numpy()
        out[f'{name}_pose_samples'] = pose_samples.numpy()
        out[f'{name}_logweights'] = logw.numpy()
        out[f'{name}_image'] = np.asarray(image, dtype=np.float32)
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=REF)
    ap.add_argument('--out', default=OUT)
    a = ap.parse_args()
    data = make(a.reference)
    np.savez(a.out, **data)
    print(a.out, {k: v.shape for k, v in data.items()})
