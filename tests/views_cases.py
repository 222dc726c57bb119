"""Cases of the view-bank tests (eogs2_amd.views, include/eogs_views.h): payload sizes, guarded allocations, the literal
restatement of the reference's view order, and the per-view Adam case. The kernels move bits, so everything here compares
bits (as int32: a NaN keeps its payload) and every tolerance on the bank itself is zero."""
import random

import torch

SENTINEL = 0x5EA75EA7  # what a guard element holds (an int32)
GUARD = 64  # guard elements (4 bytes each) on both sides of a test's table or working tensor: a multiple of 4, so 16-byte steps
V_CASES = (1, 3)
LEADS = (0, 1, 2, 3)  # floats a working tensor starts into its allocation: 0 = 16-byte aligned, else the dword path
ORDER_V = (1, 2, 5, 21)


def payloads(wg_bytes):
    """Payload sizes in floats: the small and odd ones, one that is no multiple of 4 floats, and the workgroup boundaries."""
    w = wg_bytes // 4
    return (1, 3, 4, 5, 9, 12, 1023, 1024, 1025, 3 * 33 * 65, w - 1, w, w + 1, 3 * w + 1)


def random_bits(n, seed):
    """n int32 words over the whole range: NaNs, infinities and denormals of fp32 among them."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-(1 << 31), (1 << 31) - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32)


def bits(t):
    return t.detach().contiguous().cpu().reshape(-1).view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


class Guarded:
    """An int32 allocation of GUARD + lead + n + GUARD words filled with SENTINEL; `.body` is the n words in the middle."""

    def __init__(self, n, device, lead=0):
        self.n, self.lead = n, lead
        self.all = torch.full((GUARD + lead + n + GUARD,), SENTINEL, dtype=torch.int32, device=device)
        self.body = self.all[GUARD + lead:GUARD + lead + n]

    def guards_intact(self):
        a = self.all.cpu()
        return bool((a[:GUARD + self.lead] == SENTINEL).all()) and bool((a[GUARD + self.lead + self.n:] == SENTINEL).all())


class GuardedTable:
    """V rows of `stride` bytes inside a sentinel-filled allocation, `rows_front` / `rows_back` whole guard rows around them
    in the SAME allocation (so a kernel that turned a bad order entry into an address would still write memory the test
    owns), plus GUARD words on both ends. Row payloads are set with `set_row`; the padding of a row stays SENTINEL."""

    def __init__(self, V, row_words, device, rows_front=0, rows_back=0):
        self.V, self.row_words = V, row_words
        self.stride_words = max(4, -(-row_words // 4) * 4)
        self.front = GUARD + rows_front * self.stride_words
        total = self.front + (V + rows_back) * self.stride_words + GUARD
        self.all = torch.full((total,), SENTINEL, dtype=torch.int32, device=device)

    @property
    def base(self):
        return self.all[self.front:]

    def row(self, v):
        s = self.front + v * self.stride_words
        return self.all[s:s + self.row_words]

    def set_row(self, v, words):
        self.row(v).copy_(words)

    def snapshot(self):
        return self.all.cpu().clone()

    def outside_rows_intact(self):
        """Everything but the V payloads still holds SENTINEL."""
        a = self.all.cpu().clone()
        for v in range(self.V):
            s = self.front + v * self.stride_words
            a[s:s + self.row_words] = SENTINEL
        return bool((a == SENTINEL).all())


def literal_order(n_views, iterations, seed):
    """train_pan.py:252-257 restated literally over a list of view indices, with `random` seeded as given."""
    from random import randint, seed as set_seed

    set_seed(seed)
    cameras = list(range(n_views))
    viewpoint_stack = None
    out = []
    for _ in range(iterations):
        if not viewpoint_stack:
            viewpoint_stack = cameras.copy()
        viewpoint_cam = viewpoint_stack.pop(randint(0, len(viewpoint_stack) - 1))
        out.append(viewpoint_cam)
    return out


# ---- Adam per view ----
ADAM_V = 3
ADAM_SHAPES = {"weight": (3, 3, 1, 1), "bias": (3,), "inshadow": (3, 1, 1)}  # a colour camera's parameter set
ADAM_ORDER = (0, 2, 2, 1, 2, 0, 2, 2, 0, 2, 1, 2, 2, 2, 0, 2, 0, 2, 2, 2)  # 20 iterations: 5, 2 and 13 visits
ADAM_LR, ADAM_BETAS, ADAM_EPS = 2e-3, (0.9, 0.999), 1e-8


def adam_initial(name, v):
    g = torch.Generator().manual_seed(100 + 10 * v + sorted(ADAM_SHAPES).index(name))
    return torch.randn(ADAM_SHAPES[name], generator=g)


def adam_grad(name, v, visit):
    """The gradient of parameter `name` of view v at its visit number `visit` (0-based): a fixed function of both."""
    g = torch.Generator().manual_seed(7000 + 1000 * v + 10 * visit + sorted(ADAM_SHAPES).index(name))
    return torch.randn(ADAM_SHAPES[name], generator=g) * (0.1 + 0.3 * v)


def visits(order, n_views):
    return [sum(1 for x in order if x == v) for v in range(n_views)]


def seeded(seed):
    r = random.Random()
    r.seed(seed)
    return r
