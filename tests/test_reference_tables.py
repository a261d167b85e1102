"""Pin the oracle's (and the product's) gamma tables to the literal numbers in the reference's own header.

The reference holds no golden vectors and cannot be built here, but its DeGrand-Rossi tables, gamma names and
gamma5-map are plain numeric initialisers in include/gamma.h; its displacement flags, HDF5 group formats and enumerator
values are literals too.  tests/golden/make_reference_tables.py read them out of a reference checkout AS TEXT into
tests/golden/reference_tables.json (numbers and strings only; nothing of the reference's code is stored in this
repository); these tests compare them with the oracle's restatement and with what libmugiq_hip.so reports.
"""
import json
import os
import re

import numpy as np
import pytest

from util import orc, ROOT

TABLES = os.path.join(ROOT, "tests", "golden", "reference_tables.json")


@pytest.fixture(scope="module")
def header():
    """the numbers and strings of the reference's headers (tests/golden/make_reference_tables.py)"""
    return json.load(open(TABLES))


def test_row_values_and_column_indices_equal_the_reference_header(header, hip):
    rv = np.array(header["gamma_row_value"]).reshape(16, 4, 2)                       # include/gamma.h:32-49
    ci = np.array(header["gamma_column_index"]).reshape(16, 4)                        # include/gamma.h:53-71
    ref_rv = rv[..., 0] + 1j * rv[..., 1]
    assert np.array_equal(orc.GAMMA_ROW_VALUE, ref_rv)
    assert np.array_equal(orc.GAMMA_COLUMN_INDEX, ci)
    p_rv, p_ci, p_sign, p_idx = hip.gammaTables()
    assert np.array_equal(p_rv, ref_rv) and np.array_equal(p_ci, ci)


def test_gamma_names_equal_the_reference_header(header, hip):
    names = header["gamma_names"]                                                      # include/gamma.h:13-18
    assert len(names) == 16
    assert orc.GAMMA_NAMES == names
    assert [hip.GammaName(m) for m in range(16)] == names


def test_gamma5_map_equals_the_reference_header(header, hip):
    minus = header["gamma5_map_minus"]                                                 # include/gamma.h:99-102
    assert sorted(minus) == [3, 6, 9, 11, 12, 14]
    sign = np.ones(16)
    sign[minus] = -1.0                                                                   # lib/contract_wrappers.cu:31-33
    assert np.array_equal(orc.gamma_map_sign(), sign)
    assert header["index_map_gamma"] == [15 - i for i in range(16)]                     # include/gamma.h:105-109
    assert orc.INDEX_MAP_GAMMA == [15 - i for i in range(16)]
    p_rv, p_ci, p_sign, p_idx = hip.gammaTables()
    assert np.array_equal(np.asarray(p_sign, dtype=float), sign) and list(p_idx) == [15 - i for i in range(16)]


def test_displacement_flag_table_equals_the_reference_header(header, hip):
    flags = header["displace_flags"]                                                   # include/displace.h:21
    assert flags == list(orc.DISPLACE_FLAGS)
    for i, f in enumerate(flags):                                                        # flag -> dir = flag / 2, even flag = '+'
        assert orc.parse_displacement(f) == (i // 2, orc.DISP_SIGN_PLUS if i % 2 == 0 else orc.DISP_SIGN_MINUS)
        assert hip.parseDisplacement(f) == orc.parse_displacement(f)


def test_hdf5_group_formats_equal_the_reference_source(header):
    """The on-disk tree is built from three snprintf formats and two buffer sizes (lib/loop_mugiq.cpp:581-610); the
    writer must use the same ones."""
    ours = open(os.path.join(ROOT, "mugiq_amd", "csrc", "hdf5_writer.cpp")).read()
    fmts = header["hdf5_group_formats"]
    assert fmts[:3] == ["mom_%+d_%+d_%+d", "disp_0", "disp_%s_%d"]
    for f in fmts[:3]:
        assert '"%s"' % f in ours, f
    sizes = {k: str(v) for k, v in header["hdf5_group_tag_sizes"].items()}
    assert sizes == {"group1_tag": "16", "group2_tag": "10"}
    assert dict(re.findall(r"char (group[12]_tag)\[(\d+)\]", ours)) == sizes


def test_enumerator_values_equal_the_reference_header(header, hip):
    enums = header["enums"]                                                            # include/enum_mugiq.h:29-85
    inc = open(os.path.join(ROOT, "include", "mugiq_hip.h")).read()
    mine = {k: int(v) for k, v in re.findall(r"#define (MUGIQ_HIP_[A-Z_]+) (-?\d+)\b", inc)}
    calc = enums["LoopCalcType_s"]
    assert {k: mine["MUGIQ_HIP_" + k] for k in ("LOOP_CALC_TYPE_BLAS", "LOOP_CALC_TYPE_OPT_KERNEL", "LOOP_CALC_TYPE_BASIC_KERNEL")} == \
        {k: calc[k] for k in ("LOOP_CALC_TYPE_BLAS", "LOOP_CALC_TYPE_OPT_KERNEL", "LOOP_CALC_TYPE_BASIC_KERNEL")}
    assert (hip.LOOP_CALC_TYPE_BLAS, hip.LOOP_CALC_TYPE_OPT_KERNEL, hip.LOOP_CALC_TYPE_BASIC_KERNEL) == \
        (calc["LOOP_CALC_TYPE_BLAS"], calc["LOOP_CALC_TYPE_OPT_KERNEL"], calc["LOOP_CALC_TYPE_BASIC_KERNEL"])
    d = enums["DisplaceDir_s"]
    assert [mine["MUGIQ_HIP_DISP_DIR_" + c] for c in "XYZT"] == [d["DispDir_" + c] for c in "xyzt"]
    sg = enums["DisplaceSign_s"]
    assert (mine["MUGIQ_HIP_DISP_SIGN_MINUS"], mine["MUGIQ_HIP_DISP_SIGN_PLUS"]) == (sg["DispSignMinus"], sg["DispSignPlus"])
    assert (hip.DispSignMinus, hip.DispSignPlus) == (sg["DispSignMinus"], sg["DispSignPlus"])
    assert (orc.DISP_SIGN_MINUS, orc.DISP_SIGN_PLUS) == (sg["DispSignMinus"], sg["DispSignPlus"])
    fl = enums["DisplaceFlag_s"]
    assert [fl["DispFlag_" + c] for c in "XxYyZzTt"] == list(range(8))     # the order DISPLACE_FLAGS relies on
    ft = enums["LoopFTSign_s"]
    assert (ft["LOOP_FT_SIGN_MINUS"], ft["LOOP_FT_SIGN_PLUS"]) == (-1, 1)
