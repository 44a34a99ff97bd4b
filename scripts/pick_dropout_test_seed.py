"""How tests/test_gpu_dropout.py's X_SEED was chosen (CPU only, no GPU needed).

For every candidate input seed 1..12 the test's own torch U-Net runs the gradient comparison's forward (ngf 8, bs 2,
256^2, the test's weights, seed / offset and p = 0.5, the masks from the numpy restatement of the mask function, which
the GPU export equals bit for bit) and reports the smallest nonzero |v| over the inputs of every activation at
32 x 32 and below.  The choice is the first seed whose margin is at least 1e-5, the bound the test asserts."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"),
                os.path.join(ROOT, "shadow-removal-istd_amd")]
import torch  # noqa: E402
from fixture_init import fixture_state, uniform  # noqa: E402
from stcgan_amd import engine, networks  # noqa: E402
from test_dropout_cpu import dropout_mask  # noqa: E402
import test_gpu_dropout as T  # noqa: E402

net = networks.get_generator(4, 3, ngf=T.NGF, num_downs=T.ND, use_dropout=True)
st = fixture_state(net.state_dict(), 12, "one")  # (test_gpu_dropout._net)
S = engine._sizes(256, 256, T.ND)
masks = {k: torch.from_numpy(dropout_mask(T.SEED, T.OFFSET, k, (2,) + engine._pad2(S, k) + (T.NGF * 8,), 0.5))
         .permute(0, 3, 1, 2).float() * 2 for k in (4, 5, 6)}
choice = None
for seed in range(1, 13):
    margins = []
    with torch.no_grad():
        T.unet(T._params(st), uniform((2, 4, 256, 256), seed), True, masks, margins)
    level, worst = min(margins, key=lambda t: t[1])
    print(f"seed {seed:2d}: margin {worst:.3e} (level {level})")
    if choice is None and worst >= 1e-5:
        choice = seed
print(f"X_SEED = {choice}")
assert choice == T.X_SEED, (choice, T.X_SEED)
