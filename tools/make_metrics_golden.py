"""tests/golden/metrics_eval.npz: what the reference's own evaluation functions return on fp32 poses (CPU only, needs scipy).

    python tools/make_metrics_golden.py [--reference DIR] [--check]

The functions `se3_mul ... calc_all_errs` are obtained by exec'ing the function definitions of the reference checkout's
EPro-PnP-6DoF/lib/utils/eval.py -- the span from `def se3_mul` to the end of the file, located by those markers, with numpy and
scipy injected -- the way tests/test_reference_callers.py runs reference text.  None of that text is copied anywhere; the fixture
holds data only: synthetic models (points on ellipsoids of semi-axes about 0.05 x 0.08 x 0.03 with M = 1, 257 and 1500), 40 pose
pairs per model as fp32 (t, q) / (t, yaw), intrinsics, flags, and per pose the five numbers rot_deg, trans, arp_2d (calc_all_errs),
add, adi.  The reference sees exactly what epropnp.metrics.pose_errors sees: rotation matrices of the NORMALISED fp32 quaternions /
of the fp32 yaw, formed here in fp64.

Per model: rotation offsets of 1e-3, 0.02, 0.3 and 3 rad -- six 6-DoF pairs at a depth around 1 m (LineMOD) and two 4-DoF pairs
around 50 m (the Det head's rows) each -- and eight 6-DoF half-turn pairs ('eggbox') whose raw rotation error lies between 100 and
170 degrees, clear of logm's branch point at 180.  The class name decides what calc_all_errs does: 'eggbox' symmetric with the
half-turn rule, 'glue' symmetric, 'ape' neither.
"""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'metrics_eval.npz')
MODEL_SIZES = (1, 257, 1500)
OFFSETS = (1e-3, 0.02, 0.3, 3.0)
CLASSES = ('ape', 'glue', 'eggbox')      # (symmetric, half_turn) = (0, 0), (1, 0), (1, 1)
K_LINEMOD = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], dtype=np.float32)
K_DET = np.array([[1266.4172, 0.0, 816.2670], [0.0, 1266.4172, 491.50708], [0.0, 0.0, 1.0]], dtype=np.float32)


def reference_functions(reference):
    """{name: function} of the reference's eval.py from `def se3_mul` on, exec'd from the checkout's text"""
    from scipy import spatial
    from scipy.linalg import logm
    text = open(os.path.join(reference, 'EPro-PnP-6DoF', 'lib', 'utils', 'eval.py')).read()
    start = text.index('def se3_mul')
    assert 'def calc_all_errs' in text[start:], 'eval.py: calc_all_errs not found behind se3_mul'
    ns = {'np': np, 'spatial': spatial, 'logm': logm, 'LA': np.linalg, 'math': math}
    exec(compile(text[start:], 'reference:eval.py', 'exec'), ns)
    return ns


def quat_to_rot(q):
    w, x, y, z = (np.asarray(q, dtype=np.float64) / np.linalg.norm(np.asarray(q, dtype=np.float64))).tolist()
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def yaw_to_rot(yaw):
    c, s = math.cos(float(yaw)), math.sin(float(yaw))
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def unit(rng, n):
    v = rng.standard_normal(n)
    return v / np.linalg.norm(v)


def make_inputs():
    """the fixture's inputs: deterministic, fp32"""
    rng = np.random.RandomState(20240607)
    models = [(np.stack([unit(rng, 3) for _ in range(M)]) * np.array([0.05, 0.08, 0.03])).astype(np.float32) for M in MODEL_SIZES]
    first = np.cumsum([0] + [len(m) for m in models[:-1]])
    out = {'points': np.concatenate(models, 0), 'range': np.stack([first, [len(m) for m in models]], 1).astype(np.int32)}
    rows6, rows4 = [], []
    for mid in range(len(models)):
        n = 0
        for ang in OFFSETS:
            for _ in range(6):
                rows6.append((mid, ang, CLASSES[n % 3]))
                n += 1
            for _ in range(2):
                rows4.append((mid, ang, CLASSES[n % 2]))      # 4-DoF rows: 'ape' or 'glue'
                n += 1
        for k in range(8):
            rows6.append((mid, math.radians(100.0 + 10.0 * k), 'eggbox'))
    est6, gt6, est4, gt4 = [], [], [], []
    for mid, ang, cls in rows6:
        tg = np.array([0.05, -0.03, 1.0]) + 0.1 * rng.standard_normal(3)
        qg = unit(rng, 4)
        axis = unit(rng, 3)
        qe = quat_mul(qg, np.concatenate(([math.cos(ang / 2)], math.sin(ang / 2) * axis))) * (1.0 if len(est6) % 2 else -1.0)
        te = tg + (1e-3, 5e-3, 2e-2)[len(est6) % 3] * unit(rng, 3)
        est6.append(np.concatenate((te, qe)))
        gt6.append(np.concatenate((tg, qg)))
    for mid, ang, cls in rows4:
        tg = np.array([2.0, 1.0, 50.0]) + np.array([5.0, 0.5, 5.0]) * rng.standard_normal(3)
        yg = rng.uniform(-3.0, 3.0)
        te = tg + (1e-3, 2e-2, 0.3)[len(est4) % 3] * unit(rng, 3)
        est4.append(np.concatenate((te, [yg + ang * (1.0 if len(est4) % 2 else -1.0)])))
        gt4.append(np.concatenate((tg, [yg])))
    for tag, rows, est, gt, K in (('6', rows6, est6, gt6, K_LINEMOD), ('4', rows4, est4, gt4, K_DET)):
        out['est' + tag] = np.asarray(est, dtype=np.float32)
        out['gt' + tag] = np.asarray(gt, dtype=np.float32)
        out['model_id' + tag] = np.asarray([r[0] for r in rows], dtype=np.int32)
        out['symmetric' + tag] = np.asarray([r[2] != 'ape' for r in rows], dtype=np.uint8)
        out['half_turn' + tag] = np.asarray([r[2] == 'eggbox' for r in rows], dtype=np.uint8)
        out['cam_mats' + tag] = np.repeat(K[None], len(rows), 0)
    return out


def reference_errors(inp, fns):
    """errs6 / errs4 (N,5) fp64: rot_deg, trans, arp_2d of calc_all_errs, then add and adi, on the fp32 inputs"""
    out = {}
    for tag in ('6', '4'):
        errs = []
        for i in range(len(inp['est' + tag])):
            e, g = inp['est' + tag][i].astype(np.float64), inp['gt' + tag][i].astype(np.float64)
            Re, Rg = (quat_to_rot(e[3:]), quat_to_rot(g[3:])) if tag == '6' else (yaw_to_rot(e[3]), yaw_to_rot(g[3]))
            first, count = inp['range'][inp['model_id' + tag][i]]
            pts = inp['points'][first:first + count].astype(np.float64)
            K = inp['cam_mats' + tag][i].astype(np.float64)
            cls = 'eggbox' if inp['half_turn' + tag][i] else ('glue' if inp['symmetric' + tag][i] else 'ape')
            err_r, err_t, arp, add_or_adi = fns['calc_all_errs'](Re, e[:3], Rg, g[:3], pts, K, cls)
            add, adi = fns['add'](Re, e[:3], Rg, g[:3], pts), fns['adi'](Re, e[:3], Rg, g[:3], pts)
            assert add_or_adi == (adi if cls != 'ape' else add)
            errs.append((err_r, err_t, arp, add, adi))
        out['errs' + tag] = np.asarray(errs, dtype=np.float64)
    return out


def compute(reference):
    inp = make_inputs()
    inp.update(reference_errors(inp, reference_functions(reference)))
    return inp


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('EPROPNP_REFERENCE', '/root/reference'))
    ap.add_argument('--check', action='store_true', help='compare with the committed fixture instead of writing it')
    a = ap.parse_args()
    data = compute(a.reference)
    half = data['half_turn6'] != 0
    raw = np.array([np.degrees(2 * math.atan2(np.linalg.norm(r[1:]), abs(r[0]))) for r in (
        quat_mul(e[3:] * [1, -1, -1, -1] / np.linalg.norm(e[3:]), g[3:] / np.linalg.norm(g[3:]))
        for e, g in zip(data['est6'][half].astype(np.float64), data['gt6'][half].astype(np.float64)))])
    print(f'{len(data["est6"])} 6-DoF and {len(data["est4"])} 4-DoF pose pairs; half-turn rows: raw rotation error '
          f'{raw.min():.1f} .. {raw.max():.1f} degrees, scored {data["errs6"][half][:, 0].min():.1f} .. {data["errs6"][half][:, 0].max():.1f}')
    if a.check:
        old = np.load(OUT)
        worst = max(float(np.max(np.abs(old[k].astype(np.float64) - data[k].astype(np.float64)))) for k in data)
        print(f'largest difference from {OUT}: {worst:.3e}')
        sys.exit(0 if worst <= 1e-12 else 1)
    np.savez_compressed(OUT, **data)
    print(f'wrote {OUT}: {os.path.getsize(OUT)} bytes')
