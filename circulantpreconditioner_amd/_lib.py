"""Loading of ``libcirculant_fft.so`` (the HIP/gfx950 library) and of its real-scalar build
``libcirculant_fft_real.so``; the signatures are the one table of ``_lib_ext.py``.

There is no fallback: if the shared library is missing or fails to load, every
entry point raises.  Build it with ``__graft_entry__.build()`` or
``make -C circulantpreconditioner_amd/csrc``.
"""
from __future__ import annotations

import ctypes
import os
import threading

from ._lib_ext import COMPLEX_BUILD, REAL_BUILD, PetscScalar, declare

_HERE = os.path.dirname(os.path.abspath(__file__))

# error codes (petscerror.h values), include/circulant_fft.h
CFP_SUCCESS = 0


class CirculantError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[cfp error {code}] {msg}")
        self.code = code


class _Library:
    """One of the two shared libraries: loaded on the first call, under its lock, with every
    signature of the table (_lib_ext.signatures) that its build holds.  `path` is read at that
    first call (a function: the module-level LIB_PATH / REAL_LIB_PATH as it then stands, so a tool
    may point it at another build before anything is loaded).  Raises if the file is missing:
    there is no CPU fallback."""

    def __init__(self, path, mode: int, build: str, hint: str):
        self._path, self._mode, self._build, self._hint = path, mode, build, hint
        self._lock = threading.Lock()
        self._lib = None

    def __call__(self):
        if self._lib is None:
            with self._lock:
                if self._lib is None:
                    path = self._path()
                    if not os.path.exists(path):
                        raise ImportError(f"{os.path.basename(path)} not found at {path}; build it with {self._hint}")
                    L = ctypes.CDLL(path, mode=self._mode)
                    declare(L, PetscScalar if self._build == COMPLEX_BUILD else ctypes.c_double, self._build)
                    self._lib = L
        return self._lib


LIB_PATH = os.path.join(_HERE, "lib", "libcirculant_fft.so")
REAL_LIB_PATH = os.path.join(_HERE, "lib", "libcirculant_fft_real.so")

# the complex library is RTLD_GLOBAL; the real-scalar one is RTLD_LOCAL (and linked -Bsymbolic), so
# that both live in one process
lib = _Library(lambda: LIB_PATH, ctypes.RTLD_GLOBAL, COMPLEX_BUILD,
               "`python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
real_lib = _Library(lambda: REAL_LIB_PATH, ctypes.RTLD_LOCAL, REAL_BUILD, "`make -C circulantpreconditioner_amd/csrc`")


def check(rc: int) -> None:
    if rc != CFP_SUCCESS:
        raise CirculantError(rc, lib().cfp_last_error().decode(errors="replace"))


def exported_symbols() -> list:
    """Names of every cfp_* / PETSc-boundary function the library must export."""
    names = []
    for hdr in ("circulant_fft.h", "circulant_fft_dist.h", "pcshell_fft3d.h", "petsc_mini.h",
                "transport_equation.h", "diffusion_equation.h", "wave_system.h", "circulant_fft_real.h",
                "mesh_unstructured.h", "wave_system_real.h"):
        path = os.path.join(os.path.dirname(_HERE), "include", hdr)
        if os.path.exists(path):
            names += _parse_decls(path)
    return names


def _parse_decls(path: str) -> list:
    import re
    txt = open(path).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", "", txt)
    out = []
    txt = re.sub(r"^\s*typedef[^;]*;", "", txt, flags=re.M)  # function-pointer typedefs are not exports
    for m in re.finditer(r"^\s*(?:const\s+)?[A-Za-z_][\w]*\s*\**\s*([A-Za-z_]\w*)\s*\([^;{]*\)\s*;", txt, flags=re.M):
        name = m.group(1)
        if name not in ("if", "while", "return", "sizeof") and len(name) > 2:
            out.append(name)
    return out
