"""CPU-only checks of the device-resident scene update's surface (include/grt.h: grt_update_gaussians_device): the
symbol, the ctypes mirror of grt_update_info, the Python entry points and the new kernels in the ISA budget.  No compute calls."""
import ctypes as C
import inspect
import json
import os
import re

import pytest

import grt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASM = os.path.join(ROOT, "gaussian-ray-tracing_amd", "csrc", "build_asm")
HDR = open(os.path.join(ROOT, "include", "grt.h")).read()
C_TYPES = {"uint32_t": C.c_uint32, "float": C.c_float, "uint64_t": C.c_uint64, "int32_t": C.c_int32}


def test_library_exports_the_update():
    assert "grt_update_gaussians_device" in grt.EXPORTS
    fn = grt.lib().grt_update_gaussians_device
    assert len(fn.argtypes) == 7
    m = re.search(r"GRT_API\s+int\s+grt_update_gaussians_device\s*\(([^)]*)\)", HDR)
    assert m and len(m.group(1).split(",")) == 7


def test_update_info_mirrors_the_header():
    m = re.search(r"typedef struct \{([^}]*)\}\s*grt_update_info;", HDR)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [(name, C_TYPES[typ]) for typ, name in re.findall(r"(\w+)\s+(\w+)\s*;", body)]
    assert fields == list(grt.UpdateInfo._fields_)
    assert C.sizeof(grt.UpdateInfo) == 16


def test_modes_reasons_and_option_mirror_the_header():
    def enum(name):
        m = re.search(name + r"\s*=\s*(\d+)", HDR)
        assert m, name
        return int(m.group(1))
    assert (enum("GRT_UPDATE_AUTO"), enum("GRT_UPDATE_REFIT"), enum("GRT_UPDATE_REBUILD")) == (grt.UPDATE_AUTO, grt.UPDATE_REFIT, grt.UPDATE_REBUILD)
    assert grt.UPDATE_MODES == {"auto": grt.UPDATE_AUTO, "refit": grt.UPDATE_REFIT, "rebuild": grt.UPDATE_REBUILD}
    for h, v in (("NONE", grt.REASON_NONE), ("FIRST_BUILD", grt.REASON_FIRST_BUILD), ("N_CHANGED", grt.REASON_N_CHANGED),
                 ("SET_CHANGED", grt.REASON_SET_CHANGED), ("OPTION_CHANGED", grt.REASON_OPTION_CHANGED), ("AREA", grt.REASON_AREA)):
        assert enum("GRT_UPDATE_REASON_" + h) == v
    assert enum("GRT_OPT_REFIT_MAX_AREA_PCT") == grt.OPT_REFIT_MAX_AREA_PCT
    # no other option carries that number
    assert len(re.findall(r"GRT_OPT_\w+\s*=\s*%d\b" % grt.OPT_REFIT_MAX_AREA_PCT, HDR)) == 1


def test_python_entry_points():
    sig = inspect.signature(grt.Tracer.update_device)
    assert list(sig.parameters) == ["self", "acts", "alpha_min", "mode"]
    assert sig.parameters["alpha_min"].default == 0.01 and sig.parameters["mode"].default == "auto"
    import grt_torch
    sig = inspect.signature(grt_torch.render)
    assert sig.parameters["update"].default == "auto"
    with pytest.raises(ValueError):
        grt_torch.render(None, None, None, None, None, None, None, update="sometimes")


def test_update_kernels_in_the_isa_budget():
    p = os.path.join(ASM, "isa_budget.json")
    if not os.path.exists(p):
        pytest.fail(f"{p} is missing: build() writes it (profiles/isa_budget_current.py)")
    b = {k["kernel"].split("(")[0]: k for k in json.load(open(p))["kernels"]}
    want = {"k_refit_prim_boxes": "grt_scene.s", "k_regather_records": "grt_scene.s", "k_mark_in_tree": "grt_scene.s", "k_set_changed": "grt_scene.s",
            "grt::k_child_area_partial": "grt_bvh.s"}
    for name, unit in want.items():
        assert name in b, (name, sorted(k for k in b if "render" not in k))
        k = b[name]
        # plain streaming kernels: no scratch, no spills
        assert k["file"] == unit and k["scratch_bytes"] == 0 and k["spill_instructions"] == 0, (name, k)
    # the units went through hipcc_via_asm.py unrepaired (its lint ran: build() fails otherwise)
    for unit in ("grt_api", "grt_scene", "grt_bvh"):
        assert int(open(os.path.join(ASM, unit + ".repairs.txt")).readline().split()[0]) == 0
