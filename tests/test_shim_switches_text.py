"""The drop-in's switch table (integration/c4gpu_switches.h) against the five files that read it and against INTEGRATION.md: a
text test, no binaries needed.  Every C4GPU_* token a shim file hands to an accessor is a key of the header, every key is read
somewhere, every key is documented, and no shim file names a variable in a string or reads the environment behind the table."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCESSORS = r"(?:shim_has|shim_num|shim_real|shim_is|shim_nonzero|shim_text|shim_async|SHIM_SWITCH_NAME)"


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _code(text):
    """C source without its comments."""
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def keys():
    found = re.findall(r"\bX\((C4GPU_[A-Z0-9_]+)\)", _read("integration", "c4gpu_switches.h"))
    assert len(found) == len(set(found)) >= 40
    return set(found)


def sources():
    paths = sorted(glob.glob(os.path.join(ROOT, "integration", "*.c")))
    assert len(paths) == 5
    return {os.path.basename(p): _code(_read(p)) for p in paths}


def test_every_token_passed_to_an_accessor_is_a_key():
    passed = set()
    for code in sources().values():
        passed |= set(re.findall(ACCESSORS + r"\(\s*(C4GPU_[A-Z0-9_]+)", code))
    assert passed and not (passed - keys()), sorted(passed - keys())


def test_every_key_is_read_somewhere():
    tokens = set()
    for code in sources().values():
        tokens |= set(re.findall(r"\bC4GPU_[A-Z0-9_]+\b", code))
    assert not (keys() - tokens), sorted(keys() - tokens)


def test_every_key_is_named_in_the_integration_document():
    doc = set(re.findall(r"\bC4GPU_[A-Z0-9_]+\b", _read("INTEGRATION.md")))
    assert not (keys() - doc), sorted(keys() - doc)
    assert "c4gpu_switches.h" in _read("INTEGRATION.md")


def test_no_shim_file_reads_a_switch_behind_the_table():
    for name, code in sources().items():
        strings = re.findall(r'"(?:\\.|[^"\\\n])*"', code)
        assert strings and not [s for s in strings if "C4GPU_" in s], name           # a variable named in a string
        assert "__thread" not in code and "shim_env(" not in code, name
        assert code.count("getenv(") == (1 if name == "c4gpu_shim.c" else 0), name   # the one read, before main
