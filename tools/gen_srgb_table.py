#!/usr/bin/env python3
"""Writes trace.jl_amd/csrc/th_display_srgb.h: the 255 Float32 thresholds of the display pass's sRGB encode (docs/design/18-display.md).

T[k], k = 1..255, is the smallest Float32 not below eotf((k - 0.5) / 255), the sRGB EOTF evaluated in Float64: an 8-bit code q is the number of k with t >= T[k], which is
floor(255 * oetf(t) + 0.5) without a pow at run time.  The values are written as hexadecimal Float32 literals, so the file holds the bits and no decimal rounding.

    python tools/gen_srgb_table.py            # rewrites the header
    python tools/gen_srgb_table.py --check    # exit status 1 when the committed header is not what this script writes
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "trace.jl_amd", "csrc", "th_display_srgb.h")


def eotf64(v: float) -> float:
    """IEC 61966-2-1: encoded value in [0, 1] -> linear light."""
    return v / 12.92 if v <= 0.04045 else ((v + 0.055) / 1.055) ** 2.4


def thresholds() -> np.ndarray:
    """(256,) Float32: [0] = 0, [k] = T[k]."""
    t = np.zeros(256, np.float32)
    for k in range(1, 256):
        x = eotf64((k - 0.5) / 255.0)
        f = np.float32(x)
        if float(f) < x:  # rounded down: the next Float32 up is the smallest one not below x
            f = np.nextafter(f, np.float32(np.inf), dtype=np.float32)
        assert float(f) >= x > float(np.nextafter(f, np.float32(-np.inf), dtype=np.float32))
        t[k] = f
    assert np.all(np.diff(t) > 0)
    return t


def hexf(v: np.float32) -> str:
    mantissa, exponent = float(v).hex().split("p")  # a Float32 is exactly a Float64: its hex form is exact
    return mantissa.rstrip("0") + "p" + exponent + "f"


def text() -> str:
    t = thresholds()
    lines = ["// th_display_srgb.h — written by tools/gen_srgb_table.py, not by hand: the thresholds of the display pass's sRGB encode (docs/design/18-display.md).",
             "// TH_SRGB_THRESHOLDS is 256 Float32 values: 0, then T[1] .. T[255], T[k] the smallest Float32 not below eotf((k - 0.5) / 255) of IEC 61966-2-1 evaluated in Float64;",
             f"// T[1] = {float(t[1]):.6e}, T[255] = {float(t[255]):.6f}.  The table is the specification: nothing computes it at run time.",
             "#pragma once", "// clang-format off", "#define TH_SRGB_THRESHOLDS \\"]
    vals = [hexf(v) for v in t]
    vals[0] = "0.0f"
    for i in range(0, 256, 8):
        lines.append("    " + ", ".join(vals[i:i + 8]) + ("," if i + 8 < 256 else "") + (" \\" if i + 8 < 256 else ""))
    lines.append("// clang-format on")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    if "--check" in sys.argv[1:]:
        sys.exit(0 if os.path.exists(OUT) and open(OUT).read() == text() else 1)
    open(OUT, "w").write(text())
    print(f"wrote {os.path.relpath(OUT, ROOT)}: T[1] = {float(thresholds()[1]):.6e}, T[255] = {float(thresholds()[255]):.6f}")
