"""CPU: the source list, the header list and the per-file flags of mellow_amd/csrc/build.py agree with the files they name."""
import os
import re

from mellow_amd.csrc import build

INCLUDE_DIR = os.path.normpath(os.path.join(build.HERE, "..", "..", "include"))


def _read(name):
    return open(os.path.join(build.HERE, name)).read()


def test_every_listed_file_exists():
    for name in build.SOURCES + build.HEADERS:
        assert os.path.isfile(os.path.join(build.HERE, name)), name


def test_every_project_header_a_listed_file_includes_is_in_headers():
    """An object is stale when a file of HEADERS is newer: a header missing there could be edited without its users being rebuilt."""
    listed = {os.path.normpath(os.path.join(build.HERE, h)) for h in build.HEADERS}
    for name in build.SOURCES + build.HEADERS:
        here = os.path.dirname(os.path.join(build.HERE, name))
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', _read(name), re.M):
            path = os.path.normpath(os.path.join(here, inc))
            if os.path.isfile(path) and os.path.dirname(path) in (build.HERE, INCLUDE_DIR):
                assert path in listed, f"{name} includes {inc}, which HEADERS does not list"


def test_decode_kernel_files_carry_the_kernarg_preload_flags():
    """The decode kernels put their hot pointers in front of `DecArgs a` (or take it first) so that the preloaded dwords of the
    argument block hold them; a file with such a kernel must be compiled with the flags.  (A kernel that takes another record by
    value in front of DecArgs -- the sampler, the beam merge -- is not of this form: its leading dwords are that record's.)"""
    assert build.KERNARG_PRELOAD, "run without MELLOW_KERNARG_PRELOAD=0"
    scalar = re.compile(r"\*|^\s*(const\s+)?(int|int64_t|int32_t|float)\s+\w+\s*$")
    found = []
    for name in build.SOURCES:
        if not name.endswith(".hip"):
            continue
        for m in re.finditer(r"__global__[^{;]*?\bvoid\s+\w+\s*\(([^{;]*?)\bDecArgs a\b", _read(name)):
            leading = [p for p in m.group(1).split(",") if p.strip() and p.strip() != "const"]
            if all(scalar.search(p) for p in leading):
                found.append(name)
                flags = build.FILE_FLAGS.get(name, [])
                assert all(f in flags for f in build.KERNARG_PRELOAD), name
    assert found, "no decode kernel found: the pattern of this test is out of date"
