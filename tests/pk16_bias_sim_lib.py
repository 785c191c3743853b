"""ctypes binding of build/libc4pkbias.so (tests/pk16_bias_sim.hip): the guard of the biased packed score pass
(exonerate_amd/csrc/c4_pk16_bias.h) and the kernel choice behind it, on the host.  TEST INFRASTRUCTURE: never imported by
exonerate_amd/."""
import ctypes as C
import os
import subprocess

from exonerate_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "build", "libc4pkbias.so")
CSRC = os.path.join(ROOT, "exonerate_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "pk16_bias_sim.hip")] + [os.path.join(CSRC, f) for f in
                                                            ("c4_pk16_bias.h", "c4_kernel_choice.h", "c4_launch.h", "c4_config.h")]
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
        lib.pkbias_constants.restype = None
        lib.pkbias_constants.argtypes = [C.POINTER(C.c_int)]
        lib.pkbias_fits.restype = C.c_int
        lib.pkbias_fits.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_longlong), C.c_int,
                                    C.c_longlong]
        for fn in (lib.pkbias_addend_ok, lib.pkbias_site_ok):
            fn.restype = C.c_int
            fn.argtypes = [C.c_longlong]
        lib.pkbias_choose.restype = C.c_int
        lib.pkbias_choose.argtypes = [C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int)]
        _lib = lib
    return _lib


def constants():
    out = (C.c_int * 4)()
    load().pkbias_constants(out)
    return dict(zip(("bias", "addend_max", "post_gain_max", "score_max"), out))


def fits(submat, calcs, site_worst, post_best):
    return bool(load().pkbias_fits((C.c_int * len(submat))(*submat), len(submat), (C.c_int * len(calcs))(*calcs), len(calcs),
                                   (C.c_longlong * len(site_worst))(*site_worst), len(site_worst), post_best))


def addend_ok(v):
    return bool(load().pkbias_addend_ok(v))


def site_ok(worst_sum):
    return bool(load().pkbias_site_ok(worst_sum))


def choose(qlen, n, bias_unfit):
    name = C.create_string_buffer(128)
    flags = C.c_int(0)
    err = load().pkbias_choose(qlen, n, int(bias_unfit), name, len(name), C.byref(flags))
    if err:
        return "error", name.value.decode()
    return name.value.decode(), {k for b, k in enumerate(("fmt16", "needs_ss16", "staged_codes")) if flags.value >> b & 1}
