"""zkmi — Python driver (ctypes) over the C ABI in include/zkmi.h.

This package is test/bench plumbing only: every computation happens inside
libzkmi.so (hand-written HIP for gfx950 + host C++).  There is NO CPU fallback:
if the shared library or a GPU is missing, calls raise.

The directory name contains a hyphen (the repo layout contract), so import it
through `load_pkg()` in `zkmi_loader.py` at the repo root, or via
`importlib` under the module name `zk_apps_amd`.
"""
from .binding import (  # noqa: F401
    Zkmi,
    ZkmiError,
    Context,
    lib_path,
    PHASES,
    ERR,
    ENC_WIRE,
    ENC_ZCASH_COMPRESSED,
    ENC_ZCASH_UNCOMPRESSED,
    CHECK_CURVE,
    CHECK_SUBGROUP,
    PT_OK,
    PT_BAD_ENCODING,
    PT_NOT_ON_CURVE,
    PT_NOT_IN_SUBGROUP,
    SRS_BAD_TAU_G1,
    SRS_BAD_TAU_G2,
    SRS_BAD_ALPHA,
    SRS_BAD_BETA,
    SRS_BAD_BETA_G2,
    SRS_DEGENERATE,
    SRS_STEP_BAD_TAU,
    SRS_STEP_BAD_ALPHA,
    SRS_STEP_BAD_BETA,
    SRS_STEP_DEGENERATE,
    PK2_FIXED_PART_DIFFERS,
    PK2_BAD_DELTA,
    PK2_BAD_H,
    PK2_BAD_L,
    Srs,
    ProvingKey,
    NoteTree,
)
