"""CPU: what twk_refit_instance_transform and twk_refit_instance_transforms refuse before any HIP call — a NULL handle, a NULL
transform, a batch without an entry or without its arrays: TWK_ERROR_INVALID_VALUE with a message that names the call, checkable
without a GPU (as tests/test_cabi_symbols.py checks the switches). The refusals that need a handle — before twk_build, not built in
selective mode, and every per-entry one — are tests/test_gpu_instance_refit.py's."""
import ctypes as C


def test_the_refit_calls_refuse_a_null_handle_without_touching_a_device(twk):
    L = twk._lib
    identity = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    ids = (C.c_int * 1)(0)

    def refused(rc, name, *words):
        text = L.lib.twk_last_error().decode()
        assert rc == L.TWK_ERROR_INVALID_VALUE and name in text, (rc, text)
        for w in words:
            assert w in text, text

    refused(L.lib.twk_refit_instance_transform(None, 0, identity), "twk_refit_instance_transform", "NULL device handle")
    refused(L.lib.twk_refit_instance_transform(None, 0, None), "twk_refit_instance_transform", "NULL device handle")
    refused(L.lib.twk_refit_instance_transforms(None, 1, ids, identity), "twk_refit_instance_transforms", "NULL device handle")
    # the batch's own arguments come first, as in twk_update_instance_transforms
    refused(L.lib.twk_refit_instance_transforms(None, 0, ids, identity), "twk_refit_instance_transforms", "count")
    refused(L.lib.twk_refit_instance_transforms(None, 1, None, identity), "twk_refit_instance_transforms", "NULL array")
    refused(L.lib.twk_refit_instance_transforms(None, 1, ids, None), "twk_refit_instance_transforms", "NULL array")
    # the same order and texts as the update calls make them
    for refit, update in (("twk_refit_instance_transform", "twk_update_instance_transform"), ("twk_refit_instance_transforms", "twk_update_instance_transforms")):
        texts = []
        for name in (refit, update):
            f = getattr(L.lib, name)
            rc = f(None, 0, identity) if name.endswith("transform") else f(None, -1, None, None)
            assert rc == L.TWK_ERROR_INVALID_VALUE
            texts.append(L.lib.twk_last_error().decode().replace(name, "<call>"))
        assert texts[0] == texts[1], texts
