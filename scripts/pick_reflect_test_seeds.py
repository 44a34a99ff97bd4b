"""The weight seeds of tests/test_gpu_reflect_model.py (CPU only): for each configuration the first seed whose fp64
reference keeps every activation input at least MARGIN of its own fp32 errors from zero (inorm_ref.sign_margin, a
property of the reference alone).  Prints every configuration's choice and its margin.

  python scripts/pick_reflect_test_seeds.py [first] [last]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "shadow-removal-istd_amd"), ROOT):
    sys.path.insert(0, p)
import torch  # noqa: E402

import test_gpu_reflect_model as T  # noqa: E402
from inorm_ref import sign_margin  # noqa: E402

first, last = (int(v) for v in (sys.argv[1:3] + ["1", "1500"])[:2])
torch.set_num_threads(min(16, os.cpu_count() or 1))
for cfg in T.CONFIGS:
    best = (0.0, None)
    for seed in range(first, last + 1):
        _, fresh, x = T.make(cfg, seed)
        m = sign_margin(fresh, x)
        if m > best[0]:
            best = (m, seed)
        if m >= T.MARGIN:
            print(f"{cfg}: seed {seed}, margin {m:.2f}", flush=True)
            break
    else:
        print(f"{cfg}: no seed in {first} .. {last} reaches {T.MARGIN}; best {best[1]} with {best[0]:.2f}", flush=True)
