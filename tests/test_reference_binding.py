"""The reference-side binding of INTEGRATION.md section B, driven by what the REAL reference hands its seam.

The ctypes stub a maintainer pastes into core/flash_attention_3.py is taken verbatim from INTEGRATION.md and fed the views that
every entry of the reference ending in the seam (flash_attention_3.py:97-102, modules.py:154, photonic_attention.py:385-415)
really produces: their shapes, strides (S*3E, D, 3E, 1), storage offsets and key mask were recorded from the imported reference
by oracle/make_golden.py (tests/golden/g9_seam_views.npz) and are rebuilt here over fresh storage.  `pfa_fa3_check` stands in
for the launch (no GPU here): what is verified is that the argument block the stub builds from those views passes the library's
validation unchanged."""

from __future__ import annotations

import ctypes as C
import os

import pytest
import torch

from conftest import REPO, load_golden


@pytest.fixture(scope="module")
def binding():
    from photonic_flash_attention_amd import _capi
    lib = _capi.load()
    src = open(os.path.join(REPO, "INTEGRATION.md")).read()
    code = src[src.index("class PfaFa3Args(C.Structure):"):src.index("```", src.index("def fa3_forward("))]
    code = code.replace('_lib = C.CDLL("libpfa_hip.so")', "_lib = _FAKE_LIB")
    seen = []

    class FakeLib:                        # the stub's `_lib`: same entry points, the launch replaced by the validation
        pfa_status_string = lib.pfa_status_string

        class pfa_fa3_fwd:                # (has .argtypes assigned by the stub)
            argtypes = None

            def __new__(cls, a, stream):
                args = C.cast(a, C.POINTER(_capi.PfaFa3Args)).contents
                seen.append({f: getattr(args, f) for f in ("B", "H", "Sq", "Sk", "D", "q_stride_b", "q_stride_h", "q_stride_s",
                                                           "k_stride_s", "v_stride_s", "o_stride_s", "o_stride_h", "dtype_in")})
                return lib.pfa_fa3_check(C.byref(args))
    ns = {"_FAKE_LIB": FakeLib}
    exec("import ctypes as C, torch\n" + code, ns)
    return ns["fa3_forward"], seen


def seam_views(call):
    """The q / k / v views of one recorded seam call, rebuilt over fresh storage (views that shared one keep sharing it)."""
    size = {}
    for t in ("q", "k", "v"):
        g = call[t]
        end = g["offset"] + sum((n - 1) * st for n, st in zip(g["shape"], g["stride"])) + 1
        size[g["storage"]] = max(size.get(g["storage"], 0), end)
    dt = getattr(torch, call["q"]["dtype"])
    base = {i: torch.randn(n).to(dt) for i, n in size.items()}
    return [torch.as_strided(base[call[t]["storage"]], call[t]["shape"], call[t]["stride"], call[t]["offset"]) for t in ("q", "k", "v")]


def test_stub_in_the_imported_reference(binding):
    fa3_forward, seen = binding
    meta, arr = load_golden("g9_seam_views")
    B, S, E, H, D = (meta[n] for n in ("B", "S", "E", "H", "D"))
    calls = meta["calls"]
    assert [c["entry"] for c in calls] == ["FlashAttention3.forward", "FlashAttention3.forward, 2-D attention_mask",
                                          "FlashAttention3.forward, cross attention", "PhotonicFlashAttention.forward",
                                          "PhotonicAttention._fallback_forward"]
    for i, call in enumerate(calls):
        assert not call["need_weights"]                                       # (the stub: 2-D key masks only, no attention weights)
        q, k, v = seam_views(call)
        km = None if call["mask"] is None else torch.from_numpy(arr[call["mask"]])
        assert km is None or km.dim() == 2
        out = fa3_forward(q, k, v, call["scaling"], key_mask=km)              # INTEGRATION.md, "replacement for lines 134-150"
        assert out.shape == q.shape and len(seen) == i + 1, call["entry"]
    a = seen[0]                                                               # flash_attention_3.py:85-118
    assert (a["B"], a["H"], a["Sq"], a["Sk"], a["D"]) == (B, H, S, S, D) and a["dtype_in"] == 0
    # the strided views of the fused projection (:97-99), read in place: (S*3E, D, 3E) in elements
    assert (a["q_stride_b"], a["q_stride_h"], a["q_stride_s"]) == (S * 3 * E, D, 3 * E)
    assert a["k_stride_s"] == 3 * E and a["v_stride_s"] == 3 * E
    assert (a["o_stride_h"], a["o_stride_s"]) == (D, E)                       # [B,S,H,D] output: the transpose at :107 is a view
    km = arr[calls[1]["mask"]]                                                # the 2-D key mask of :166-167
    assert km.shape == (B, S) and (km[:, :100] == 1).all() and (km[:, 100:] == 0).all()
    assert seen[2]["Sk"] == 77 * 8 and seen[2]["k_stride_s"] == 3 * E         # cross attention: three separate projections (:92-94)
    # modules.py:77-116 -> gpu_attention and photonic_attention.py:385-415 end in the same views
    for a in seen[3:]:
        assert (a["q_stride_b"], a["q_stride_h"], a["q_stride_s"]) == (S * 3 * E, D, 3 * E)


def test_stub_reports_library_errors(binding):
    fa3_forward, _ = binding
    q = torch.zeros(1, 2, 64, 48, dtype=torch.bfloat16)                       # head dim 48: PFA_ERR_HEAD_DIM through the stub
    with pytest.raises(RuntimeError, match="head dim"):
        fa3_forward(q, q, q, 48 ** -0.5)
