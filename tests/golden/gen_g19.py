"""Freeze fixture g19: outputs of the reference's own histogram_match_rgb (s2_emit/color.py:55-63, loaded with
oracle/ref_loader.load_color) on the float32 images of tests/hist_cases.py.  Run where the reference tree lies:

    python tests/golden/gen_g19.py

The inputs are not stored: hist_cases.image_case(name) rebuilds them from its seed, and the fixture keeps a CRC of their bytes, so a
generator that drifts shows as a CRC mismatch, not as a wrong output.  Every masked sample of every case is finite: what np.unique does
with NaN is not claimed."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import hist_cases as hc                  # noqa: E402
from oracle import ref_loader            # noqa: E402


def main():
    color = ref_loader.load_color()
    out = {}
    for name in hc.IMAGE_CASES:
        src, ref, mask = hc.image_case(name)
        got = color.histogram_match_rgb(src.copy(), ref.copy(), mask.copy())
        assert got.dtype == np.float32 and got.shape == src.shape
        out["out/" + name] = got
        out["crc/" + name] = np.uint32(hc.input_crc(name))
    path = os.path.join(HERE, "g19_histmatch_f32.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 100 * 1024, size
    print(f"wrote {path}: {size} bytes, {len(hc.IMAGE_CASES)} cases")


if __name__ == "__main__":
    main()
