"""The scene validator (csrc/hrt_scene_pack.hip: check_nodes, validate_and_pack) through the host-only test hook
hrt_debug_validate_scene -- no GPU.  It is all that stands between a caller's malformed arrays and a GPU fault, so every one of its
15 rejection paths is named here: a small valid scene passes, and one minimal mutation per path (tests/scene_mutations.py) is
rejected with that path's text.  The validator returns the first thing it finds, so the exact text also says that nothing earlier
in its order objected to the mutated scene.

Message 6 ("array too long for 32-bit indices") is reached with a count alone: validate_and_pack compares the 15 counts with
0x7FFFFFF0 before it reads any element, so a count above it over the scene's own (short, non-NULL) array is never dereferenced."""
import ctypes as C

import pytest

from ilgpu_raytracing_amd import _types as T
from tests import scene_mutations as M

OK, ERR_INVALID_ARG = 0, -1          # HRT_OK, HRT_ERR_INVALID_ARG (include/hip_raytrace.h)


@pytest.fixture(scope="module")
def valid():
    return M.valid_arrays()


def _validate(lib, desc, cap=256):
    lib.hrt_debug_validate_scene.argtypes = [C.POINTER(T.SceneDesc), C.c_char_p, C.c_int]
    msg = C.create_string_buffer(b"\xff" * cap, cap)
    rc = lib.hrt_debug_validate_scene(C.byref(desc), msg, cap)
    return rc, msg.value.decode()


def test_the_valid_scene_passes(hooks_lib, valid):
    desc, keep = T.scene_desc_from_arrays(valid)
    assert _validate(hooks_lib, desc) == (OK, "")
    assert hooks_lib.hrt_debug_validate_scene(C.byref(desc), None, 0) == OK          # the text is optional


@pytest.mark.parametrize("name", list(M.MUTATIONS))
def test_each_rejection_path_names_itself(hooks_lib, valid, name):
    before = {k: v.copy() for k, v in valid.items()}
    desc, keep, message = M.mutated_desc(valid, name)
    assert _validate(hooks_lib, desc) == (ERR_INVALID_ARG, message)
    assert all((valid[k] == before[k]).all() for k in valid), "the shared valid scene was mutated"


@pytest.mark.parametrize("array", [name for name, _ in T.SCENE_ARRAYS])
def test_array_too_long_for_32_bit_indices(hooks_lib, valid, array):
    desc, keep = T.scene_desc_from_arrays(valid)
    setattr(desc, "n_" + array, M.TOO_LONG)
    assert _validate(hooks_lib, desc) == (ERR_INVALID_ARG, "array too long for 32-bit indices")


def test_every_message_of_the_validator_is_covered():
    texts = {m.split(": ")[-1] for _, m in M.MUTATIONS.values()} | {"array too long for 32-bit indices"}
    assert len(texts) == 15
    for what in ("tlasNodes", "blasNodes"):
        got = {m.split(": ")[1] for _, m in M.MUTATIONS.values() if m.startswith(what + ": ")}
        assert got == {"skipIndex out of range", "leaf range outside the index list", "left child out of range", "node links form a cycle"} \
            | ({"skipIndex below its BLAS"} if what == "blasNodes" else set())


def test_a_short_buffer_gets_a_terminated_prefix(hooks_lib, valid):
    desc, keep, message = M.mutated_desc(valid, "tlas_cycle")
    assert _validate(hooks_lib, desc, cap=10) == (ERR_INVALID_ARG, message[:9])
