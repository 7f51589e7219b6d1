"""Alignment refusals of the C-ABI, and the allocation seams of ops.py (no GPU needed: nothing here launches a kernel).

Every pointer a kernel reads or writes with 8- or 16-byte vector accesses must be refused by its entry point with
IPSR_ERR_INVALID, before any HIP call, when it is not aligned: a contiguous batch-slice view `x[1:]` or an `out=` slice at an
odd offset reaches the entries unchecked by the Python wrappers.  The calls below use FAKE device addresses (never
dereferenced: the refusal comes first) and run in a child process with every GPU hidden, so that an entry which lost its check
fails to launch instead of launching on a misaligned address.
"""
import ast
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IPSR_ERR_INVALID = -1

# fake device addresses: one 1 MiB-aligned slot per pointer argument
_BASE = 1 << 40


def _addr(slot):
    return _BASE + slot * (1 << 20)


WS = 1 << 40          # workspace bytes: never the refusal here


def _P(p, name, slot):
    return p.get(name, _addr(slot))


# entry -> (argument builder: {pointer name: address} -> ctypes args, [(pointer, offset in bytes, why)])
# Offsets are the largest misalignment below the requirement that is still a whole element (4 bytes of fp32, 2 of bf16 -> we use
# 4 or 8 bytes), so a refusal keyed on the element size alone would not pass.
CASES = [
    # conv_bf16.hip: A / input fragments are 16-byte reads (load_x of conv_bf16x3_kernel and conv_bf16x3_s2_kernel, the LDS-DMA of
    # conv_bf16_kernel); the bf16 tile leaves as uint4 rows (conv_bf16_kernel's epilogue); the split reduction reads and stores 4-element
    # vectors (cb_split_reduce_kernel)
    ("ipsr_conv3x3_bf16_packed",
     lambda p: (0, _P(p, "in", 0), _P(p, "weight", 1), _P(p, "out", 2), 2, 32, 16, 16, 48, 1, 0, _P(p, "ws", 3), WS, None),
     [("in", 8, "conv_bf16_kernel: 16-byte fragment reads"), ("out", 8, "conv_bf16_kernel epilogue: uint4 store of the bf16 tile"),
      ("out", 4, "conv_bf16_kernel epilogue"), ("ws", 8, "packed weights read as uint4")]),
    ("ipsr_conv3x3_bf16",
     lambda p: (2, _P(p, "in", 0), _P(p, "weight", 1), _P(p, "out", 2), 2, 64, 32, 64, 48, 0, _P(p, "ws", 3), WS, None),
     [("out", 8, "cb_split_reduce_kernel: st4 of the split reduction (fp32 out)"), ("in", 4, "conv_bf16x3_kernel load_x")]),
    ("ipsr_conv4x4s2_bf16",
     lambda p: (0, _P(p, "in", 0), _P(p, "weight", 1), _P(p, "out", 2), 2, 48, 32, 16, 16, 1, _P(p, "ws", 3), WS, None),
     [("out", 8, "conv_bf16_kernel epilogue: uint4 store of the fine -> coarse bf16 tile"), ("in", 8, "conv_bf16_kernel dma_x"), ("ws", 8, "packed weights")]),
    ("ipsr_conv4x4s2_bf16_wrw",
     lambda p: (_P(p, "fine", 0), _P(p, "coarse", 1), _P(p, "dw", 2), 2, 48, 32, 16, 16, _P(p, "ws", 3), WS, None),
     [("fine", 8, "16-byte row reads"), ("coarse", 8, "16-byte row reads"), ("dw", 8, "cb_slab_reduce_kernel<16>: float4 store")]),
    ("ipsr_conv3x3_bf16_wrw",
     lambda p: (0, _P(p, "x", 0), _P(p, "dy", 1), _P(p, "dw", 2), 2, 32, 16, 16, 48, _P(p, "ws", 3), WS, None),
     [("x", 8, "16-byte fragment reads"), ("dy", 8, "16-byte fragment reads"), ("ws", 8, "workspace vectors")]),
    # winograd.hip: wino_input_kernel reads a window's inner four columns as one ld4 when W % 4 == 0; the tile output stores
    # st4 (wino_output_kernel); the polyphase filter transforms read each 4x4 weight as four float4 (wino52_filter_kernel,
    # wino52_filter_split_kernel); the k4 weight gradients store float4 (wino_wrw_output4_kernel)
    ("ipsr_conv3x3_winograd_mp",
     lambda p: (0, _P(p, "in", 0), _P(p, "weight", 1), None, 0, _P(p, "filter_cache", 4), 0, _P(p, "out", 2), 2, 32, 16, 16, 48, 0, 0,
                _P(p, "ws", 3), WS, None),
     [("in", 8, "wino_input_kernel: ld4 of fp32 activations"), ("out", 8, "wino_output_kernel: st4"), ("filter_cache", 8, "transformed filter vectors"),
      ("ws", 8, "workspace vectors")]),
    ("ipsr_conv3x3_winograd_mp",              # bf16 activations in (io = 1): a vector is 8 bytes
     lambda p: (1, _P(p, "in", 0), _P(p, "weight", 1), None, 0, None, 0, _P(p, "out", 2), 2, 32, 16, 16, 48, 0, 1, _P(p, "ws", 3), WS, None),
     [("in", 4, "wino_input_kernel: ld4 of bf16 activations (8 bytes)")]),
    ("ipsr_conv4x4s2_winograd_mp",
     lambda p: (0, _P(p, "a", 0), _P(p, "b", 1), _P(p, "out", 2), 2, 32, 16, 8, 8, 0, 0, _P(p, "ws", 3), WS, None),
     [("b", 8, "wino52_filter_kernel: float4 reads of the weight"), ("b", 4, "wino52_filter_kernel"), ("out", 8, "output vectors"), ("ws", 8, "workspace")]),
    ("ipsr_conv4x4s2_winograd_mp",            # coarse -> fine under the split-bf16 arithmetic: the split filter transform
     lambda p: (1, _P(p, "a", 0), _P(p, "b", 1), _P(p, "out", 2), 2, 32, 16, 8, 8, 2, 0, _P(p, "ws", 3), WS, None),
     [("b", 8, "wino52_filter_split_kernel: float4 reads of the weight")]),
    ("ipsr_conv4x4_winograd_mp",
     lambda p: (0, 2, _P(p, "a", 0), _P(p, "b", 1), _P(p, "out", 2), 2, 32, 16, 16, 48, 0, 0, _P(p, "ws", 3), WS, None),
     [("out", 8, "wino_wrw_output4_kernel: float4 store of the weight gradient"), ("ws", 8, "workspace")]),
    ("ipsr_conv_smallmap",
     lambda p: (2, _P(p, "a", 0), _P(p, "b", 1), _P(p, "out", 2), 2, 128, 128, 4, 4, 8, 8, 4, 2, 1, 1, _P(p, "ws", 3), WS, None),
     [("a", 8, "operand vectors"), ("b", 8, "the weight read in place as a GEMM operand"), ("out", 8, "output vectors")]),
    # thin_conv.hip: few -> many stores pixel pairs (:33-34); many -> few reads ld4 (:120) and stores st4 (:141); the stream weight
    # gradient reads ld4 (:171, :187); the matrix-core few -> many stores uint4 (:575); the matrix-core weight gradient reads 16-byte
    # fragments of the wide tensor
    ("ipsr_conv3x3_thin_io",
     lambda p: (0, _P(p, "in", 0), _P(p, "w", 1), None, 0, _P(p, "out", 2), 2, 3, 64, 32, 48, 27, 9, 0, 0, None),
     [("out", 4, "thin_conv.hip:33 float2 store of a pixel pair")]),
    ("ipsr_conv3x3_thin_io",
     lambda p: (1, _P(p, "in", 0), _P(p, "w", 1), None, 0, _P(p, "out", 2), 2, 128, 3, 24, 32, 9, 27, 1, 0, None),
     [("in", 8, "thin_conv.hip:120 ld4"), ("out", 8, "thin_conv.hip:141 st4")]),
    ("ipsr_conv3x3_thin_wrw_io",
     lambda p: (_P(p, "big", 0), _P(p, "small", 1), _P(p, "g", 2), 2, 64, 3, 32, 48, 0, _P(p, "ws", 3), WS, None),
     [("big", 8, "thin_conv.hip:171 ld4"), ("small", 8, "thin_conv.hip:187 ld4"), ("ws", 8, "workspace")]),
    ("ipsr_conv_thin_f2m_mfma",
     lambda p: (_P(p, "in", 0), _P(p, "w", 1), None, 0, _P(p, "out", 2), 2, 3, 64, 16, 32, 4, 2, 48, 16, 0, 2, None),
     [("out", 8, "thin_conv.hip:575 uint4 store")]),
    ("ipsr_conv_thin_wrw_mfma",
     lambda p: (_P(p, "big", 0), _P(p, "small", 1), _P(p, "g", 2), 2, 64, 3, 16, 32, 4, 2, 1, _P(p, "ws", 3), WS, None),
     [("big", 8, "16-byte fragment reads of the wide tensor"), ("ws", 8, "workspace")]),
    ("ipsr_conv2d",
     lambda p: (0, _P(p, "in", 0), _P(p, "weight", 1), _P(p, "out", 2), 2, 32, 16, 16, 48, 3, 1, 1, 1, _P(p, "ws", 3), WS, None),
     [("ws", 8, "packed operand vectors")]),
    # api.hip: the layer and its parts
    ("ipsr_corr_argmax",
     lambda p: (_P(p, "xn", 0), _P(p, "ref", 1), 2, 64, 256, _P(p, "ind", 2), _P(p, "vmax", 3), None, _P(p, "ws", 4), WS, None),
     [("xn", 8, "float4 tiles"), ("ref", 8, "float4 tiles")]),
    ("ipsr_corr_argmax_bf16",
     lambda p: (_P(p, "xn", 0), _P(p, "ref", 1), 2, 64, 256, _P(p, "ind", 2), _P(p, "vmax", 3), _P(p, "ws", 4), WS, None),
     [("xn", 8, "float4 tiles"), ("ref", 8, "float4 tiles"), ("ws", 8, "bf16 operand vectors")]),
    ("ipsr_forward",
     lambda p: (_P(p, "x", 0), _P(p, "ref", 1), _P(p, "mpi", 5), 16, 2, 64, 16, 16, 1, 1, _P(p, "out", 2), _P(p, "ind", 6), _P(p, "vmax", 7),
                None, None, _P(p, "ws", 3), WS, None),
     [("x", 8, "float4 rows"), ("ref", 8, "float4 rows"), ("out", 8, "float4 stores"), ("ws", 8, "workspace")]),
    # glue kernels (pointwise.hip / instnorm.hip): one 4-element vector per lane when the plane is a multiple of 4
    ("ipsr_bias_act",
     lambda p: (_P(p, "x", 0), _P(p, "bias", 1), 2, 8, 64, 1, 0.2, 0, None, None),
     [("x", 8, "fp32 vectors of 16 bytes")]),
    ("ipsr_bias_act",
     lambda p: (_P(p, "x", 0), _P(p, "bias", 1), 2, 8, 64, 1, 0.2, 1, None, None),
     [("x", 4, "bf16 vectors of 8 bytes")]),
    ("ipsr_bias_act_skip",
     lambda p: (_P(p, "x", 0), _P(p, "bias", 1), 2, 8, 64, 1, 0.2, 0, _P(p, "y2", 2), 16 * 64, None, None),
     [("y2", 8, "the skip destination is stored as vectors")]),
    ("ipsr_cat_relu_forward",
     lambda p: (_P(p, "y", 0), _P(p, "x", 1), 2, 8, 8, 64, 0, _P(p, "out", 2), None),
     [("y", 8, "vectors"), ("x", 8, "vectors"), ("out", 8, "vectors")]),
    ("ipsr_cat_relu_backward",
     lambda p: (_P(p, "g", 0), _P(p, "out", 1), 2, 8, 8, 64, 0, _P(p, "dy", 2), _P(p, "dx", 3), None),
     [("g", 8, "vectors"), ("out", 8, "vectors"), ("dy", 8, "vectors"), ("dx", 8, "vectors")]),
    ("ipsr_instnorm_act_forward",
     lambda p: (_P(p, "x", 0), None, None, None, 1e-5, 1, 0.2, 2, 8, 64, 0, _P(p, "y", 1), _P(p, "mean", 2), _P(p, "rstd", 3), _P(p, "tickets", 4), None),
     [("x", 8, "vectors"), ("y", 8, "vectors")]),
    ("ipsr_bias_act_backward",
     lambda p: (_P(p, "dy", 0), _P(p, "y", 1), 1, 0.2, 2, 8, 64, 0, _P(p, "dx", 2), None, None, None, None),
     [("dy", 8, "vectors"), ("y", 8, "vectors"), ("dx", 8, "vectors")]),
    ("innercos_loss",
     lambda p: (_P(p, "x", 0), 2, 8, 8, 64, _P(p, "mask", 1), _P(p, "target", 2), 1.0, _P(p, "loss", 3), _P(p, "ws", 4), WS, None),
     [("x", 8, "float4 reads"), ("mask", 8, "float4 reads"), ("target", 8, "float4 reads")]),
]


def _case_ids():
    return ["%s[%d]:%s+%d" % (entry, i, ptr, off) for i, (entry, _, rows) in enumerate(CASES) for ptr, off, _ in rows]


def _child():
    """Runs with every GPU hidden: call each entry with one misaligned fake pointer, report (rc, message)."""
    sys.path.insert(0, ROOT)
    from deepinpainting_amd import _lib
    L = _lib.lib()
    out = {}
    for i, (entry, build, rows) in enumerate(CASES):
        for ptr, off, _why in rows:
            args = build({})
            base = build({ptr: None})          # locate the pointer's position: the builder default is a distinct slot
            pos = [k for k, (a, b) in enumerate(zip(args, base)) if a != b]
            assert len(pos) == 1, (entry, ptr)
            a = list(args)
            a[pos[0]] = args[pos[0]] + off
            rc = getattr(L, entry)(*a)
            out["%s[%d]:%s+%d" % (entry, i, ptr, off)] = (rc, L.ipsr_last_error().decode("utf-8", "replace"))
    print(json.dumps(out))


@pytest.fixture(scope="module")
def refusals():
    import __graft_entry__ as g
    g.build()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("case", _case_ids())
def test_misaligned_vector_operand_is_refused(refusals, case):
    rc, msg = refusals[case]
    assert rc == IPSR_ERR_INVALID and "align" in msg, "%s: status %d, %r" % (case, rc, msg)


def test_every_vector_entry_family_is_audited():
    """The table covers each entry family whose kernels make vector accesses (a new conv engine needs a row)."""
    entries = {c[0] for c in CASES}
    for must in ("ipsr_conv3x3_bf16_packed", "ipsr_conv4x4s2_bf16", "ipsr_conv4x4s2_bf16_wrw", "ipsr_conv3x3_bf16_wrw",
                 "ipsr_conv3x3_winograd_mp", "ipsr_conv4x4s2_winograd_mp", "ipsr_conv4x4_winograd_mp", "ipsr_conv_smallmap",
                 "ipsr_conv3x3_thin_io", "ipsr_conv3x3_thin_wrw_io", "ipsr_conv_thin_f2m_mfma", "ipsr_conv_thin_wrw_mfma", "ipsr_forward"):
        assert must in entries


def test_ops_allocates_through_the_seams():
    """deepinpainting_amd/ops.py allocates every result, cache and ticket through `_empty` / `_zeros` and every scratch buffer
    through `_workspace`, so the guarded-memory tests (tests/guarded.py) see each buffer a kernel touches."""
    src = open(os.path.join(ROOT, "deepinpainting_amd", "ops.py")).read()
    tree = ast.parse(src)
    seams = {"_empty", "_zeros", "_workspace"}
    banned = {"empty", "zeros", "empty_like", "zeros_like", "ones", "full", "empty_strided", "new_empty", "new_zeros", "new_full"}
    bad = []

    class V(ast.NodeVisitor):
        def __init__(self):
            self.fn = []

        def visit_FunctionDef(self, node):
            self.fn.append(node.name)
            self.generic_visit(node)
            self.fn.pop()

        def visit_Call(self, node):
            f = node.func
            name = f.attr if isinstance(f, ast.Attribute) else (f.id if isinstance(f, ast.Name) else None)
            if name in banned and not (self.fn and self.fn[0] in seams):
                bad.append("ops.py:%d %s" % (node.lineno, ast.get_source_segment(src, node)[:60]))
            self.generic_visit(node)

    V().visit(tree)
    assert not bad, "allocations outside the seams: %s" % bad


if __name__ == "__main__" and sys.argv[1:] == ["--child"]:
    _child()
