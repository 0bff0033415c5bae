"""cmdg_mrigark_desc: the ctypes mirror (climatemachine.jl_amd/_lib.py) keeps include/cmdg.h's field
order, and the MRI constants agree (no GPU needed)."""
import os
import re

from cmdg_loader import cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "cmdg.h")).read()


def test_mrigark_desc_matches_header_field_order():
    txt = header()
    body = txt[txt.index("typedef struct cmdg_mrigark_desc {"):txt.index("} cmdg_mrigark_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).replace("typedef struct cmdg_mrigark_desc {", "")
    fields = []
    for stmt in body.split(";"):
        stmt = " ".join(stmt.split())
        if stmt:
            for nm in re.sub(r"^(const\s+)?\w+\s+", "", stmt).split(","):
                nm = re.sub(r"\[.*\]", "", nm).replace("*", "").strip()
                if nm:
                    fields.append(nm)
    assert fields == [f[0] for f in cm._lib.CmdgMrigarkDesc._fields_], fields


def test_mrigark_constants_match_header():
    txt = header()
    L = cm._lib
    assert "#define CMDG_MRI_MAXR %d" % L.MRI_MAXR in txt
    assert "#define CMDG_MRI_MAXGAMMA %d" % L.MRI_MAXGAMMA in txt
    assert "#define CMDG_MRIGARK_EXPLICIT %d" % L.MRIGARK_EXPLICIT in txt
    assert "#define CMDG_MRIGARK_DECOUPLED_IMPLICIT %d" % L.MRIGARK_DECOUPLED_IMPLICIT in txt


def test_new_entries_are_bound():
    names = {s[0] for s in cm._lib.SYMBOLS}
    assert {"cmdg_mri_lsrk_update", "cmdg_mri_qhat", "cmdg_mrigark_step"} <= names
