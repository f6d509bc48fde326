"""Write tests/golden/sinc_ref.json by RUNNING the reference's two sinc functions:

  python3 tools/make_golden_sinc.py REFERENCE_CHECKOUT [OUT]

`make_sinc_coefficients` (gateware/bbb/sinc.py) and `do_interpolation` (gateware/bbb/tests/test_sinc.py) are read from the
reference checkout at run time; their modules import migen and matplotlib, so the two function definitions are taken out
with `ast` and executed on their own, with two stand-ins for names that newer libraries dropped:
  np.int               -> int            (removed from current numpy)
  scipy.signal.hamming -> numpy.hamming  (removed from current scipy in favour of scipy.signal.windows.hamming; the two
                                          differ by one ulp and quantise to the same int8 table)
The fixture holds data only: the 32 packed BRAM words, the 72 input samples of the reference's test (its own expression
for them, evaluated by do_interpolation's first two lines and rebuilt here from the same formula), and the 1106 values
do_interpolation returns."""
import ast
import json
import pathlib
import sys
import types

import numpy as np

OUT = pathlib.Path(__file__).resolve().parent.parent / "tests" / "golden" / "sinc_ref.json"


def grab(path, name):
    src = pathlib.Path(path).read_text()
    for node in ast.parse(src).body:
        if isinstance(node, ast.FunctionDef) and node.name == name:
            return ast.get_source_segment(src, node)
    raise KeyError(f"{name} not found in {path}")


class _Numpy:
    """numpy with the alias the reference still uses"""

    def __getattr__(self, k):
        return int if k == "int" else getattr(np, k)


def main(ref, path=OUT):
    ref = pathlib.Path(ref)
    g = {"np": _Numpy(), "scipy": types.SimpleNamespace(signal=types.SimpleNamespace(hamming=np.hamming))}
    exec(grab(ref / "gateware" / "bbb" / "sinc.py", "make_sinc_coefficients"), g)
    exec(grab(ref / "gateware" / "bbb" / "tests" / "test_sinc.py", "do_interpolation"), g)
    packed = [int(w) for w in g["make_sinc_coefficients"]()]
    out = [int(v) for v in g["do_interpolation"]()]
    x = (np.sin(2 * np.pi * 7 * np.linspace(0, 1, 72)) * 127).astype(np.int8)     # the test's input memory
    assert len(packed) == 32 and len(out) == 1106
    doc = {"source": "make_sinc_coefficients() of gateware/bbb/sinc.py and do_interpolation() of gateware/bbb/tests/test_sinc.py, executed",
           "packed": packed, "input": x.tolist(), "output": out}
    pathlib.Path(path).write_text(json.dumps(doc) + "\n")


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(*sys.argv[1:])
