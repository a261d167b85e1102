#!/usr/bin/env python3
"""Regenerates tests/golden/reference_tables.json from a checkout of the reference (ckallidonis/mugiq).

The reference holds no golden vectors, but its DeGrand-Rossi tables, gamma names, gamma5-map, displacement flags,
HDF5 group formats and enumerator values are plain initialisers and literals in its headers and lib/loop_mugiq.cpp.
This script reads those files AS TEXT and stores only the extracted numbers and strings, so that
tests/test_reference_tables.py pins the oracle and the product to them without the reference tree being present.

usage: python tests/golden/make_reference_tables.py <reference-tree> > tests/golden/reference_tables.json
"""
import json
import os
import re
import sys


def _ints(block):
    return [int(v) for v in re.findall(r"-?\d+", re.sub(r"//[^\n]*", "", block))]


def _initialiser(src, name):
    """the brace-balanced initialiser that follows `name[...][...] =`"""
    i = src.index(name)
    i = src.index("=", i)
    j = src.index("{", i)
    depth, k = 0, j
    while True:
        depth += {"{": 1, "}": -1}.get(src[k], 0)
        k += 1
        if depth == 0:
            break
    return src[j:k]


def _c_enum(src, name):
    """name -> {enumerator: value} of a C enum in `src` (implicit values count up from the previous one)"""
    body = re.search(r"typedef enum %s\s*\{(.*?)\}" % name, re.sub(r"//[^\n]*", "", src), re.S).group(1)
    out, nxt = {}, 0
    for item in [x.strip() for x in body.split(",") if x.strip()]:
        if "=" in item:
            k, v = [t.strip() for t in item.split("=")]
            if not re.fullmatch(r"-?\d+", v):
                continue                                                   # "= MUGIQ_INVALID_ENUM"
            nxt = int(v)
        else:
            k = item
        out[k] = nxt
        nxt += 1
    return out


def extract(ref):
    gamma = open(os.path.join(ref, "include", "gamma.h")).read()
    displace = open(os.path.join(ref, "include", "displace.h")).read()
    loop = open(os.path.join(ref, "lib", "loop_mugiq.cpp")).read()
    enums = open(os.path.join(ref, "include", "enum_mugiq.h")).read()

    block = gamma[gamma.index("gNames"):]
    names = [n.strip() for n in re.findall(r'"([^"]*)"', block[:block.index("}")])]     # include/gamma.h:13-18
    minus = _ints(re.search(r"minusG\s*\{([^}]*)\}", gamma).group(1))                     # include/gamma.h:99-102
    n_gamma = len(names)
    idx_rule = re.search(r"idxG\.at\(i\)\s*=\s*N_GAMMA_\s*-\s*i\s*-\s*1", gamma)           # include/gamma.h:105-109
    flags = re.findall(r'"([^"]*)"', re.search(r"DisplaceFlagArray\s*\{([^}]*)\}", displace).group(1))   # include/displace.h:21
    fmts = re.findall(r'snprintf\(\s*group\d_tag\s*,\s*sizeof\(group\d_tag\)\s*,\s*"([^"]*)"', loop)    # lib/loop_mugiq.cpp:581-610
    sizes = {k: int(v) for k, v in re.findall(r"char (group[12]_tag)\[(\d+)\]", loop)}
    return {
        "source": "ckallidonis/mugiq: include/gamma.h, include/displace.h, include/enum_mugiq.h, lib/loop_mugiq.cpp",
        "gamma_row_value": _ints(_initialiser(gamma, "rowValue[")),                      # include/gamma.h:32-49, [16][4][re, im]
        "gamma_column_index": _ints(_initialiser(gamma, "columnIdx[")),                  # include/gamma.h:53-71, [16][4]
        "gamma_names": names,
        "gamma5_map_minus": minus,
        "index_map_gamma": [n_gamma - i - 1 for i in range(n_gamma)] if idx_rule else None,
        "displace_flags": flags,
        "hdf5_group_formats": fmts[:3],
        "hdf5_group_tag_sizes": sizes,
        "enums": {e: _c_enum(enums, e) for e in ("LoopCalcType_s", "DisplaceDir_s", "DisplaceSign_s", "DisplaceFlag_s",
                                                 "LoopFTSign_s")},                       # include/enum_mugiq.h:29-85
    }


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    json.dump(extract(sys.argv[1]), sys.stdout, indent=1)
    sys.stdout.write("\n")
