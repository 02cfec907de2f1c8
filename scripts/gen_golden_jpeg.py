"""Writes tests/golden/jpeg_kat.npz: six small JPEG files (Pillow's encoder: the three samplings, grayscale,
restart markers, optimised tables, a box-replicated chroma plane) as byte arrays file_0..file_5, each with
the RGB array rgb_k that Pillow's decoder gave for it when the fixture was made, and the versions that made it.
tests/test_crosscity.py and tests/test_gpu_crosscity.py hold both decodes to the recording, so a Pillow /
libjpeg of another machine that decodes differently shows up as a difference instead of moving the oracle.

    python scripts/gen_golden_jpeg.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import jpeg_ref  # noqa: E402


def main():
    import PIL
    from PIL import features
    out = {"versions": np.array([f"Pillow {PIL.__version__}", f"libjpeg-turbo {features.version('libjpeg_turbo')}"])}
    for k, data in enumerate(jpeg_ref.golden_cases()):
        out[f"file_{k}"] = np.frombuffer(data, np.uint8)
        out[f"rgb_{k}"] = jpeg_ref.pillow_rgb(data)
    path = os.path.join(ROOT, "tests", "golden", "jpeg_kat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", ", ".join(out["versions"]))


if __name__ == "__main__":
    main()
