"""The switches on the per-hit shading are stated once in the Python layer (_SWITCHES, DESIGN.md "One switch table in the host layers"); every
other layer must carry each row: the header, the library's exports, load_library, both renderers' methods and both constructors.  No device."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The parameter lists of include/mirt.h, by kind of row: a scalar switch (bool or int) and the per-material table (list).
HEADER_PARAMS = {
    "scalar": ("mirt_set_{n}(mirt_ctx* ctx, uint32_t {v});", "mirt_get_{n}(const mirt_ctx* ctx, uint32_t* {v});", "mirt_group_set_{n}(mirt_group* group, uint32_t {v});"),
    "table": ("mirt_set_{n}(mirt_ctx* ctx, const uint8_t* closure, uint32_t n);",
              "mirt_get_{n}(const mirt_ctx* ctx, uint8_t* closure_out, uint32_t capacity, uint32_t* n, uint32_t* mixed);",
              "mirt_group_set_{n}(mirt_group* group, const uint8_t* closure, uint32_t n);"),
}
VALUE_NAME = {"light_ris": "candidates"}                   # every other scalar switch calls its value `on`

# The two constructors as they stood before the table: parameter lists, order and defaults.
RENDERER = ("(scene: 'Scene', device: 'int' = 0, max_bounces: 'int' = 16, buckets: 'int' = 5, mis: 'bool' = True, use_bvh: 'bool' = False, "
            "count_traffic: 'bool' = False, profile: 'bool' = False, max_batch: 'int' = 0, allow_half_boxes: 'bool' = True, reference_tree: 'bool' = False, "
            "streams: 'int' = 0, gpu_build: 'bool' = False, trace_primary_rays: 'bool' = False, brdf: 'int' = 0, gloss_decay=None, "
            "exact_stream_order: 'bool' = False, aov: 'bool' = False, lens: 'bool' = False, light_ris: 'int' = 0, transmission: 'bool' = False, "
            "sky_sampling: 'bool' = False, material_closures=None, ggx_pdf: 'bool' = False)")
GROUP_RENDERER = ("(scene: 'Scene', devices=(0,), max_bounces: 'int' = 16, buckets: 'int' = 5, mis: 'bool' = True, use_bvh: 'bool' = True, "
                  "count_traffic: 'bool' = False, max_batch: 'int' = 0, streams: 'int' = 0, reference_tree: 'bool' = False, gpu_build: 'bool' = False, "
                  "brdf: 'int' = 0, gloss_decay=None, exact_stream_order: 'bool' = False, aov: 'bool' = False, lens: 'bool' = False, light_ris: 'int' = 0, "
                  "transmission: 'bool' = False, sky_sampling: 'bool' = False, material_closures=None, ggx_pdf: 'bool' = False)")


def test_the_table_holds_the_switches(mirt):
    assert {"ggx_pdf", "light_ris", "material_closures", "sky_sampling", "transmission"} <= {name for name, _, _ in mirt._SWITCHES}
    assert all(kind in (bool, int, list) for _, kind, _ in mirt._SWITCHES)


def test_constructors_are_the_parents(mirt):
    assert str(inspect.signature(mirt.Renderer)) == RENDERER
    assert str(inspect.signature(mirt.GroupRenderer)) == GROUP_RENDERER


def test_every_layer_carries_every_row(mirt):
    for row in mirt._SWITCHES:
        carries(mirt, *row)


def carries(mirt, name, kind, default):
    header = open(os.path.join(ROOT, "include", "mirt.h")).read()
    lib, raw = mirt.load_library(), C.CDLL(mirt.LIB_PATH)
    for decl in HEADER_PARAMS["table" if kind is list else "scalar"]:
        decl = decl.format(n=name, v=VALUE_NAME.get(name, "on"))
        assert re.search(r"^int " + re.escape(decl), header, flags=re.M), f"include/mirt.h does not declare: int {decl}"
    for symbol in (f"mirt_set_{name}", f"mirt_get_{name}", f"mirt_group_set_{name}"):
        assert hasattr(raw, symbol), f"{symbol} is not exported by libmirt.so"
        assert symbol in lib._declared, f"{symbol} is not declared by load_library"
        assert getattr(lib, symbol).argtypes is not None and getattr(lib, symbol).restype is C.c_int
    assert getattr(lib, f"mirt_set_{name}")(None, *((None, 0) if kind is list else (1,))) < 0           # NULL context: MIRT_ERR_ARG, no device touched
    assert getattr(lib, f"mirt_group_set_{name}")(None, *((None, 0) if kind is list else (1,))) < 0
    for cls in (mirt.Renderer, mirt.GroupRenderer):
        assert inspect.isfunction(getattr(cls, "set_" + name)) and getattr(cls, "set_" + name).__doc__, f"{cls.__name__}.set_{name}"
        assert inspect.isfunction(getattr(cls, name)), f"{cls.__name__}.{name}"                           # a method, not a property
        assert name not in cls.__dict__, f"{cls.__name__} carries a getter of its own for {name}"        # one implementation, in the shared base
        parameter = inspect.signature(cls).parameters[name]
        assert parameter.default is default or parameter.default == default and type(parameter.default) is type(default)
