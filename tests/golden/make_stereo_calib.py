"""Extract the stereo rectification block of the reference's
Examples/Stereo/EuRoC.yaml (:37-81, LEFT.* and RIGHT.*: height, width, D, K,
R, P) with the Camera.* values a stereo Frame needs (fx, fy, cx, cy, bf,
width, height) -> tests/golden/euroc_stereo_calib.json. Settings only: numbers
parsed from text with their full printed precision (repr round-trips a double),
nothing from the file is executed.

    python tests/golden/make_stereo_calib.py <reference>/Examples/Stereo/EuRoC.yaml

Run once where the reference is at hand; the .json is committed."""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "euroc_stereo_calib.json")


def matrix(txt, key):
    m = re.search(re.escape(key) + r":\s*!!opencv-matrix\s+rows: (\d+)\s+cols: (\d+)\s+dt: d\s+data:\s*\[([^\]]*)\]", txt)
    rows, cols = int(m.group(1)), int(m.group(2))
    v = [float(t) for t in m.group(3).replace("\n", " ").split(",")]
    assert len(v) == rows * cols, key
    return v


def scalar(txt, key):
    return float(re.search(r"^" + re.escape(key) + r":\s*(\S+)", txt, re.M).group(1))


def main():
    txt = open(sys.argv[1]).read()
    out = {}
    for side in ("LEFT", "RIGHT"):
        out[side + ".height"] = int(scalar(txt, side + ".height"))
        out[side + ".width"] = int(scalar(txt, side + ".width"))
        for k in ("D", "K", "R", "P"):
            out[f"{side}.{k}"] = matrix(txt, f"{side}.{k}")
    for k in ("fx", "fy", "cx", "cy", "bf"):
        out["Camera." + k] = scalar(txt, "Camera." + k)
    for k in ("width", "height"):
        out["Camera." + k] = int(scalar(txt, "Camera." + k))
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(len(out), "keys ->", OUT)


if __name__ == "__main__":
    main()
