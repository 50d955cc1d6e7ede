"""The C ABI of the differentiable field normal (include/vsrd_hip.h: vsrd_field_eval_adjoint), met without a device: the symbol and its
prototype, and every refusal that happens before a launch -- those vsrd_field_eval_backward makes, side by side with it, and the one of
its own (no cotangent at all) -- checked with null pointers and made-up addresses, which a call that refuses never follows."""
import ctypes

import pytest

DUMMY = 4096                     # a made-up non-null address: a refused call reads nothing behind it


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from vsrd_amd import _lib
    return _lib.load()


def _field(num_instances=3, temperature=0.4, instances=DUMMY, mlp_weights=None):
    from vsrd_amd import _lib
    return _lib.Field(num_instances, temperature, instances, mlp_weights)


def _adjoint(lib, field, num_points=300, workspace_bytes=None, hard=0, **changes):
    """vsrd_field_eval_adjoint with made-up addresses everywhere; `changes` name arguments to pass as given (None: a null pointer)."""
    N = 1 if field is None else field.num_instances
    need = lib.vsrd_workspace_bytes(N, 1 if field is not None and field.mlp_weights else 0)
    p = lambda name, default=DUMMY: changes.get(name, default)
    return lib.vsrd_field_eval_adjoint(field, p("positions"), num_points, p("grad_distances"), p("grad_labels", None if hard else DUMMY),
                                       p("grad_gradients"), hard, p("workspace"), need if workspace_bytes is None else workspace_bytes,
                                       p("grad_positions"), p("grad_instances"), p("grad_mlp_weights", None), None)


def _backward(lib, field, num_points=300, workspace_bytes=None, hard=0, **changes):
    """The same call of vsrd_field_eval_backward (which has no grad_gradients)."""
    N = 1 if field is None else field.num_instances
    need = lib.vsrd_workspace_bytes(N, 1 if field is not None and field.mlp_weights else 0)
    p = lambda name, default=DUMMY: changes.get(name, default)
    return lib.vsrd_field_eval_backward(field, p("positions"), num_points, p("grad_distances"), p("grad_labels", None if hard else DUMMY), hard,
                                        p("workspace"), need if workspace_bytes is None else workspace_bytes, p("grad_positions"),
                                        p("grad_instances"), p("grad_mlp_weights", None), None)


def test_symbol_and_prototype(lib):
    from vsrd_amd import _lib
    assert "vsrd_field_eval_adjoint" in _lib.SIGNATURES and hasattr(lib, "vsrd_field_eval_adjoint")
    void, size, i32, i64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int32, ctypes.c_int64
    field = ctypes.POINTER(_lib.Field)
    assert _lib.SIGNATURES["vsrd_field_eval_adjoint"] == (i32, [field, void, i64, void, void, void, i32, void, size, void, void, void, void])
    # the old entry keeps its prototype: the new one with grad_gradients taken out
    assert _lib.SIGNATURES["vsrd_field_eval_backward"] == (i32, [field, void, i64, void, void, i32, void, size, void, void, void, void])
    assert lib.vsrd_abi_version() == 12                          # added within ABI 12: probe for the symbol


def test_refusals_of_the_old_entry(lib):
    """Every refusal vsrd_field_eval_backward makes before a launch, made by both entries."""
    for call in (_adjoint, _backward):
        _refusals(lib, call)


def _refusals(lib, call):
    from vsrd_amd import _lib
    invalid, short = _lib.E_INVALID_ARGUMENT, _lib.E_WORKSPACE
    assert call(lib, None) == invalid                                                    # no field
    assert call(lib, _field(instances=None)) == invalid                                  # a field without instances
    for N in (0, -1, 65, 1 << 20):                                                       # N outside 1 .. 64
        assert call(lib, _field(num_instances=N), workspace_bytes=1 << 30) == invalid
    for T in (0.0, -0.4):
        assert call(lib, _field(temperature=T)) == invalid
    assert call(lib, _field(), positions=None) == invalid                                # points but no positions
    assert call(lib, _field(), num_points=-1) == invalid
    assert call(lib, _field(), grad_instances=None) == invalid
    assert call(lib, _field(), hard=1, grad_labels=DUMMY) == invalid                     # label cotangents exist for the soft union only
    residual = _field(mlp_weights=DUMMY)
    assert call(lib, residual, grad_mlp_weights=None) == invalid                         # a residual field needs somewhere for the MLP's gradient
    for field, extra in [(_field(), {}), (_field(num_instances=1), {}), (_field(num_instances=64), {}), (residual, dict(grad_mlp_weights=DUMMY))]:
        need = lib.vsrd_workspace_bytes(field.num_instances, 1 if field.mlp_weights else 0)
        assert need > 0
        assert call(lib, field, workspace_bytes=need - 1, **extra) == short
        assert call(lib, field, workspace_bytes=0, **extra) == short
        assert call(lib, field, workspace=None, **extra) == short
    # the residual workspace is the larger one: the box-only size does not serve a residual field
    assert call(lib, residual, workspace_bytes=lib.vsrd_workspace_bytes(3, 0), grad_mlp_weights=DUMMY) == short


def test_no_cotangent_is_refused(lib):
    """At least one of the three cotangents: the new entry's own refusal (the old one accepts such a call and returns zeros)."""
    from vsrd_amd import _lib
    none = dict(grad_distances=None, grad_labels=None, grad_gradients=None)
    assert _adjoint(lib, _field(), **none) == _lib.E_INVALID_ARGUMENT
    assert _adjoint(lib, _field(), hard=1, **none) == _lib.E_INVALID_ARGUMENT
    assert _adjoint(lib, _field(mlp_weights=DUMMY), grad_mlp_weights=DUMMY, **none) == _lib.E_INVALID_ARGUMENT
    assert _adjoint(lib, _field(), num_points=0, **none) == _lib.E_INVALID_ARGUMENT
    # ... before anything else is looked at: with a short workspace it is still the arguments that are wrong
    assert _adjoint(lib, _field(), workspace_bytes=0, **none) == _lib.E_INVALID_ARGUMENT
    # any single one passes this check and gets as far as the workspace check
    for name in none:
        if name == "grad_labels":
            one = dict(none, grad_labels=DUMMY)
            assert _adjoint(lib, _field(), workspace_bytes=0, **one) == _lib.E_WORKSPACE
            continue
        for hard in (0, 1):
            one = dict(none, **{name: DUMMY})
            assert _adjoint(lib, _field(), hard=hard, workspace_bytes=0, **one) == _lib.E_WORKSPACE
