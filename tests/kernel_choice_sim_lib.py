"""ctypes binding of build/libc4kchoice.so (tests/kernel_choice_sim.hip): the product's kernel choice
(exonerate_amd/csrc/c4_kernel_choice.h) with the real kernel table behind it, on the host.  TEST INFRASTRUCTURE: never
imported by exonerate_amd/."""
import ctypes as C
import os
import subprocess

from exonerate_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "build", "libc4kchoice.so")
CSRC = os.path.join(ROOT, "exonerate_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "kernel_choice_sim.hip")] + [os.path.join(CSRC, f)
                                                                 for f in ("c4_kernel_choice.h", "c4_launch.h", "c4_config.h")]
FAMILY = {"affine": 1, "est2genome": 2, "protein2dna": 4, "protein2genome": 5, "ner": 31}      # c4k::Family
SCORE, PATH, REGION, CKPT = 0, 1, 2, 3                                               # c4k's MODE_*
FACTS = ("family", "mode", "cont", "n", "blocked", "span", "local", "local_exact", "starts_pack", "cont_free", "seed_mode",
         "kshift", "fmt16", "pk16_params_ok", "pk16_all_fit", "tdense_n", "ss16_built", "cu_count")
SWITCHES = ("MW", "WPE", "PACK", "PK16", "PK16_IO", "PK16_C8", "PK16_R6", "PK16_LONG", "PK16_NW8", "WIN16", "WIN_NW", "CK16",
            "CK16_ROOT")
DEFAULT = -2 ** 31
_lib = None


def load():
    global _lib
    if _lib is None:
        if (not os.path.exists(SO)) or os.path.getmtime(SO) < max(os.path.getmtime(x) for x in SRC):
            os.makedirs(os.path.dirname(SO), exist_ok=True)
            subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "--offload-host-only", "-O1", "-std=c++17",
                                   "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, SRC[0], "-o", SO,
                                   "-L" + os.path.join(ROOT, "exonerate_amd"), "-lc4gpu",
                                   "-Wl,-rpath," + os.path.join(ROOT, "exonerate_amd")])
        _abi.load()
        lib = C.CDLL(SO)
        lib.kcsim_choose.restype = C.c_int
        lib.kcsim_choose.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_char_p, C.c_int,
                                     C.POINTER(C.c_int)]
        lib.kcsim_ck16_rooted.restype = None
        lib.kcsim_ck16_rooted.argtypes = [C.c_longlong, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_char_p, C.c_int]
        lib.kcsim_pk16_enabled.restype = C.c_int
        lib.kcsim_pk16_enabled.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        lib.kcsim_geometry.restype = C.c_int
        lib.kcsim_geometry.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                       C.c_char_p, C.c_int, C.POINTER(C.c_int)]
        _lib = lib
    return _lib


def _switches(switches):
    unknown = set(switches) - set(SWITCHES)
    assert not unknown, unknown
    return (C.c_int * len(SWITCHES))(*[switches.get(k, DEFAULT) for k in SWITCHES])


def choose(query_lengths, switches=None, **facts):
    """(kernel name, {"fmt16", "needs_ss16", "staged_codes"} that are set), or ("error", text).  query_lengths: one per job
    (n = their count), or (length, n) for n jobs alike; facts: LaunchFacts members by name, the others 0."""
    if isinstance(query_lengths, tuple):
        query_lengths = [query_lengths[0]] * query_lengths[1]
    unknown = set(facts) - set(FACTS)
    assert not unknown, unknown
    facts.setdefault("n", len(query_lengths))
    f = (C.c_int * len(FACTS))(*[int(facts.get(k, 0)) for k in FACTS])
    send = [] if facts.get("cont") else query_lengths            # Engine::run_impl lists them for launches without continuation
    q = (C.c_int * max(1, len(send)))(*send)
    name = C.create_string_buffer(128)
    flags = C.c_int(0)
    err = load().kcsim_choose(f, _switches(switches or {}), q, len(send), name, len(name), C.byref(flags))
    if err:
        return "error", name.value.decode()
    return name.value.decode(), {k for b, k in enumerate(("fmt16", "needs_ss16", "staged_codes")) if flags.value >> b & 1}


GEOMETRY = ("R", "waves", "hbm_carry", "staged_rows", "staged_rows6")
PK16, WIN16, CK16, CK16_ROOTED = 1, 2, 3, 4               # kcsim_geometry's `which` for a kernel named by its form


def _geometry(which, family, index, query_lengths, switches, facts):
    facts.setdefault("n", len(query_lengths))
    f = (C.c_int * len(FACTS))(*[int(facts.get(k, 0)) for k in FACTS])
    send = [] if facts.get("cont") else query_lengths
    q = (C.c_int * max(1, len(send)))(*send)
    name = C.create_string_buffer(128)
    geo = (C.c_int * len(GEOMETRY))()
    err = load().kcsim_geometry(which, family, index, f, _switches(switches or {}), q, len(send), name, len(name), geo)
    out = dict(zip(GEOMETRY, geo))
    out["name"] = None if err else name.value.decode()
    out["error"] = name.value.decode() if err else None
    return out


def geometry(query_lengths, switches=None, **facts):
    """The kernel choose() names for the same arguments, with its geometry from the kernel table: {"name", "R" (query rows per
    lane), "waves" (per job), "hbm_carry", "staged_rows", "staged_rows6" (pk16_staged_rows / _rows6), "error"}; name is None
    and error the text where the launch cannot be served."""
    if isinstance(query_lengths, tuple):
        query_lengths = [query_lengths[0]] * query_lengths[1]
    unknown = set(facts) - set(FACTS)
    assert not unknown, unknown
    return _geometry(0, 0, 0, query_lengths, switches, dict(facts))


def form_geometry(which, family, index):
    """The same for a kernel of the packed passes named by its form: which = PK16 (index: c4k::Pk16Form), WIN16 (Win16Shape), CK16
    (Ck16Shape) or CK16_ROOTED (Ck16RootedShape); name None where the family has no such kernel."""
    return _geometry(which, FAMILY[family], index, [], None, {})


def ck16_rooted(strips, n_rooted, rows_max, switches=None):
    name = C.create_string_buffer(128)
    load().kcsim_ck16_rooted(strips, n_rooted, rows_max, _switches(switches or {}), name, len(name))
    return name.value.decode()


def pk16_enabled(family, params_ok, n_jobs, switches=None):
    return bool(load().kcsim_pk16_enabled(FAMILY[family], int(params_ok), n_jobs, _switches(switches or {})))
