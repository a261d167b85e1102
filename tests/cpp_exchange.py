"""The case directory tests/cpp/operators.cpp and the Python tests exchange (tests/test_gpu_cpp_operators.py, tests/test_cpp_operators_cpu.py).

manifest.txt has one line per object: its kind, then key=value tokens in a fixed order --

  spinor    name file precision order X volumeCB stride parity_offset
  coarse    name file precision nSpin nColor X volumeCB stride parity_offset
  gauge     name file precision X R stride parity_offset
  clover    name file precision X volumeCB stride parity_offset
  transfer  name file precision nVec geoBlockSize spinBlockSize X stride parity_offset
  coarseop  name file precision nVec X volumeCB kappa hasClover
  scalars   name values

-- every descriptor member of the struct in include/mugiq_hip.h (nParity is always 2).  `file` holds the raw bytes of the DEVICE buffer of
the mugiq_amd field object as it is, pads and NaN-filled pads included, so that the C++ program and the Python binding see identical bytes
in identical layouts ("-": no bytes, the descriptor alone).  Doubles are written as C's %a (float.hex) and round-trip exactly.

results.txt, written by the program: "d NAME v..." (doubles, %a), "i NAME v..." (integers), "s NAME HEX" (text, hex-encoded) and
"buf <a manifest line>" for every output buffer, whose bytes are in the file the line names."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "operators.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "operators_cpp_test")


def build():
    """tests/cpp/operators.cpp -> tests/cpp/operators_cpp_test, the way tests/test_cpp_host.py builds loop.cpp (no oracle library)"""
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), SRC, "-o", EXE,
                           "-L", os.path.join(ROOT, "mugiq_amd"), "-lmugiq_hip", "-Wl,-rpath," + os.path.join(ROOT, "mugiq_amd")])


def build_if_stale():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(os.path.join(ROOT, "include", "mugiq_hip_operators.hpp"))):
        build()


KEYS = {"spinor": ("precision", "order", "X", "volumeCB", "stride", "parity_offset"),
        "coarse": ("precision", "nSpin", "nColor", "X", "volumeCB", "stride", "parity_offset"),
        "gauge": ("precision", "X", "R", "stride", "parity_offset"),
        "clover": ("precision", "X", "volumeCB", "stride", "parity_offset"),
        "transfer": ("precision", "nVec", "geoBlockSize", "spinBlockSize", "X", "stride", "parity_offset"),
        "coarseop": ("precision", "nVec", "X", "volumeCB", "kappa", "hasClover"),
        "scalars": ("values",)}
_LISTS = ("X", "R", "geoBlockSize")


def describe(obj):
    """(kind, descriptor dict) of a mugiq_amd field object, member for member from its desc()"""
    d, kind = obj.desc(), type(obj).__name__
    if kind == "SpinorField":
        assert d.nParity == 2
        return "spinor", dict(precision=d.precision, order=d.field_order, X=list(d.X), volumeCB=d.volumeCB, stride=d.stride, parity_offset=d.parity_offset)
    if kind == "CoarseField":
        return "coarse", dict(precision=d.precision, nSpin=d.nSpin, nColor=d.nColor, X=list(d.X), volumeCB=d.volumeCB, stride=d.stride,
                              parity_offset=d.parity_offset)
    if kind == "GaugeField":
        return "gauge", dict(precision=d.precision, X=list(d.X), R=list(d.R), stride=d.stride, parity_offset=d.parity_offset)
    if kind == "CloverField":
        return "clover", dict(precision=d.precision, X=list(d.X), volumeCB=d.volumeCB, stride=d.stride, parity_offset=d.parity_offset)
    if kind == "Transfer":
        return "transfer", dict(precision=d.precision, nVec=d.nVec, geoBlockSize=list(d.geoBlockSize), spinBlockSize=d.spinBlockSize, X=list(d.X),
                                stride=d.stride, parity_offset=d.parity_offset)
    if kind == "CoarseOperator":
        return "coarseop", dict(precision=d.precision, nVec=d.nVec, X=list(d.X), volumeCB=d.volumeCB, kappa=float(d.kappa), hasClover=d.hasClover)
    raise TypeError(kind)


def device_bytes(obj):
    """the device buffer of a field object as it is, copied to the host: uint8"""
    t = obj.V if type(obj).__name__ == "Transfer" else obj.data
    return t.detach().cpu().contiguous().numpy().view(np.uint8).reshape(-1)


def _token(key, v):
    if key in _LISTS:
        return ",".join(str(int(x)) for x in v)
    if key == "values":
        return ",".join(float(x).hex() for x in v) if len(v) else "-"
    if key == "kappa":
        return float(v).hex()
    return str(int(v))


def line(kind, name, desc, file="-"):
    head = [kind, "name=" + name] + ([] if kind == "scalars" else ["file=" + file])
    return " ".join(head + ["%s=%s" % (k, _token(k, desc[k])) for k in KEYS[kind]])


def parse_line(text):
    """(kind, name, file, descriptor dict) of a manifest line"""
    tok = text.split()
    kind, kv = tok[0], dict(t.split("=", 1) for t in tok[1:])
    desc = {}
    for k in KEYS[kind]:
        v = kv[k]
        if k in _LISTS:
            desc[k] = [int(x) for x in v.split(",")]
        elif k == "values":
            desc[k] = [] if v == "-" else [float.fromhex(x) for x in v.split(",")]
        elif k == "kappa":
            desc[k] = float.fromhex(v)
        else:
            desc[k] = int(v)
    return kind, kv["name"], kv.get("file", "-"), desc


def read_manifest(path):
    with open(path) as f:
        return [parse_line(t) for t in f if t.strip()]


class CaseWriter:
    """Collects the objects of a case and writes manifest.txt and one file of raw bytes per object into `directory`."""

    def __init__(self, directory):
        self.dir, self.lines, self.names = str(directory), [], set()
        os.makedirs(self.dir, exist_ok=True)

    def _add(self, name, text):
        assert name not in self.names and " " not in name, name
        self.names.add(name)
        self.lines.append(text)

    def field(self, name, obj):
        kind, desc = describe(obj)
        device_bytes(obj).tofile(os.path.join(self.dir, name + ".bin"))
        self._add(name, line(kind, name, desc, name + ".bin"))
        return obj

    def descriptor(self, name, kind, desc):
        """an object without bytes (what --parse-only round-trips)"""
        self._add(name, line(kind, name, desc))

    def scalars(self, name, values):
        self._add(name, line("scalars", name, dict(values=[float(v) for v in np.asarray(values, dtype=np.float64).reshape(-1)])))

    def close(self):
        with open(os.path.join(self.dir, "manifest.txt"), "w") as f:
            f.write("\n".join(self.lines) + "\n")


class Results:
    """results.txt of a run: .d[name] float64 arrays, .i[name] int64 arrays, .s[name] text, .buf[name] = (kind, descriptor, uint8 bytes)"""

    def __init__(self, directory):
        self.d, self.i, self.s, self.buf = {}, {}, {}, {}
        with open(os.path.join(str(directory), "results.txt")) as f:
            for text in f:
                tag, _, rest = text.rstrip("\n").partition(" ")
                if tag == "buf":
                    kind, name, file, desc = parse_line(rest)
                    self.buf[name] = (kind, desc, np.fromfile(os.path.join(str(directory), file), dtype=np.uint8))
                    continue
                tok = rest.split()
                if tag == "d":
                    self.d[tok[0]] = np.array([float.fromhex(x) for x in tok[1:]], dtype=np.float64)
                elif tag == "i":
                    self.i[tok[0]] = np.array([int(x) for x in tok[1:]], dtype=np.int64)
                elif tag == "s":
                    self.s[tok[0]] = bytes.fromhex(tok[1] if len(tok) > 1 else "").decode()
                else:
                    raise ValueError("results.txt: " + text)

    def z(self, name):
        """doubles as complex pairs"""
        return self.d[name].view(np.complex128)
