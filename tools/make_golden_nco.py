"""Write tests/golden/nco_rom.json: the NCO's ROM from the restated formula of gateware/bbb/nco.py:30-31,
round_half_even(32767 * sin(t_i)) with t = linspace(0, 2 pi, 1024)."""
import json
import pathlib
import sys

import numpy as np

OUT = pathlib.Path(__file__).resolve().parent.parent / "tests" / "golden" / "nco_rom.json"


def main(path=OUT):
    t = np.linspace(0, 2 * np.pi, 1024)
    v = np.sin(t) * 32767
    rom = np.round(v).astype(np.int64)
    margin = float(np.min(np.abs(np.abs(v - np.floor(v)) - 0.5)))     # distance of every entry from a half-integer
    doc = {"formula": "round_half_even(32767 * sin(2 * pi * i / 1023)), i = 0..1023 (np.linspace(0, 2 pi, 1024))",
           "n": 24, "m": 10, "p": 16, "min_distance_from_half": round(margin, 6), "rom": rom.tolist()}
    pathlib.Path(path).write_text(json.dumps(doc) + "\n")


if __name__ == "__main__":
    main(*sys.argv[1:])
