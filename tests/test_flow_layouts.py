"""CPU: the workspace layouts of the flow network's fused update blocks and encoders, pinned as literals. The eogs_*_bytes and
eogs_*_hidden_offset entries run without a device; the values are those of the library before the two update blocks and the
two encoders were folded into one table-driven implementation each (csrc/flownet.hip, csrc/flowenc.hip), so a change of
either description, of the carving or of the packing plan shows here. One column moved on purpose: RAFT-small's CONTEXT
encoder no longer carves the buffers only its FEATURE kind touches, and its sizes fell by exactly that memory."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from eogs2_amd import build

    build.build(verbose=False)
    from eogs2_amd import _lib

    return _lib.get()


# (N, h, w): flownet_update_bytes, flownet_update_hidden_offset, flowlarge_bytes, flowlarge_hidden_offset
UPDATE = {
    (1, 1, 1): (4098560, 4094976, 18115840, 18110976),
    (1, 16, 16): (5093376, 4388608, 20072192, 18894336),
    (2, 17, 19): (6616064, 4837888, 23064320, 20092416),
    (3, 5, 40): (6436352, 4784896, 22711552, 19951104),
    (1, 128, 128): (68057088, 22968064, 143806208, 68439552),
    (1, 256, 256): (259946496, 79591168, 520900352, 219434496),
}

# (N, H, W): flowenc_bytes FEATURE, flowres_bytes FEATURE, flowenc_bytes CONTEXT before the fold, flowres_bytes CONTEXT
# (None: refused, the feature encoder's last map is a single position)
ENCODER = {
    (1, 9, 8): (387328, 5892608, 405760, 10018304),
    (1, 8, 8): (None, None, 403200, 10014464),
    (2, 33, 47): (830720, 6801664, 849152, 10710272),
    (1, 128, 136): (2762496, 10782976, 2780928, 13760768),
    (2, 200, 264): (14859008, 35678464, 14877440, 32810240),
    (1, 1024, 1024): (144029440, 301566208, 144047872, 236493056),
    (1, 2048, 2048): (574994176, 1188661504, 575012608, 915970304),
}


def test_update_block_layouts(lib):
    n = ctypes.c_size_t()
    for shape, want in UPDATE.items():
        got = []
        for entry in (lib.flownet_update_bytes, lib.flownet_update_hidden_offset, lib.flowlarge_bytes, lib.flowlarge_hidden_offset):
            lib.check(entry(*shape, ctypes.byref(n)))
            got.append(n.value)
        assert tuple(got) == want, shape


def small_context_dropped(N, H, W):
    """What RAFT-small's CONTEXT plan carved and no launch of that kind touched, each piece rounded up to 256 bytes as the
    carving does: r3 (the third convolution's map, the size of a block's output), four (mean, rstd) tables of the widest
    map and the partial sums (16 x 8 tiles x channels x (sum, sum of squares) in double, at the level where that is most)."""
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    sizes, (h, w) = [], (H, W)
    for width in (32, 64, 96):
        h, w = (h + 1) // 2, (w + 1) // 2
        sizes.append((N * h * w * width, N * ((w + 15) // 16) * ((h + 7) // 8) * width))
    return up(4 * max(s[0] for s in sizes)) + 4 * up(4 * N * 96 * 2) + up(8 * 2 * max(s[1] for s in sizes))


def test_encoder_layouts(lib):
    from eogs2_amd._abi import FLOWENC_CONTEXT, FLOWENC_FEATURE

    n = ctypes.c_size_t()
    for shape, (small_f, large_f, small_c, large_c) in ENCODER.items():
        for entry, kind, want in ((lib.flowenc_bytes, FLOWENC_FEATURE, small_f), (lib.flowres_bytes, FLOWENC_FEATURE, large_f),
                                  (lib.flowenc_bytes, FLOWENC_CONTEXT, small_c - small_context_dropped(*shape)),
                                  (lib.flowres_bytes, FLOWENC_CONTEXT, large_c)):
            if want is None:
                assert entry(*shape, kind, ctypes.byref(n)) == -1, (shape, kind)
            else:
                lib.check(entry(*shape, kind, ctypes.byref(n)))
                assert n.value == want, (shape, kind)
