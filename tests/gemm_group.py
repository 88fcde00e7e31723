"""Helper (not a test) of tests/test_gemm_group_gpu.py and tests/test_gemm_plan_cpu.py: the grouped and the slab-summing split-K GEMM entry
points of include/hsad.h (hsad_gemm_nt_bf16_group_splitk, hsad_gemm_nt_bf16_splitk, hsad_gemm_nt_bf16_splitk_acc) held to an fp64 CPU product.

* GroupItem mirrors `hsad_gemm_group_item` field for field (tests/test_gemm_plan_cpu.py compares the layout with the C compiler's).
* core_plan / plain_plan / workspace_floats / tile_orders restate the host-side planning (csrc/hsad_gemm_plan.h, g8_launch) in Python.
* Operands.  EXACT: A, B integers in [-4, 4] as bf16, a pre-filled C integers in [-1024, 1024]; make_case asserts
  max|A| max|B| K + max|C0| < 2^24 on the tensors it made, so every partial sum in any order is an integer fp32 holds exactly and the
  result must EQUAL the fp64 product whatever the k order, the range cut and the slab order.  ROUNDED: randn * 0.5 and randn / sqrt(K).
* Poison, for every case: A is allocated [M + 8, K + 8] and B [N + 8, K + 16] with NaN in the padding columns and in the 8 extra rows (a
  read past K or past row N - 1 stays inside the buffer and shows in the result wherever it reaches a column that is stored); the workspace is
  NaN before each call (a slab element nobody wrote surfaces as NaN) and 1,024 floats longer than asked for, the tail holding a bit pattern
  that must survive; C is a canvas of canary words in which only the payload (rows named by row_map, columns < n_out) is pre-filled -- with
  NaN for accumulate = 0 (proves it overwrites), with the integer fill for accumulate = 1 -- and everything else is compared bitwise."""
import ctypes as C

import numpy as np
import torch

DEV = "cuda:0"
HSAD_ERR_INVALID = -1
WS_TAIL = 1024
TILE_K = 64


class GroupItem(C.Structure):
    """hsad_gemm_group_item (include/hsad.h)"""
    _fields_ = [("A", C.c_void_p), ("B", C.c_void_p), ("C", C.c_void_p), ("row_map", C.c_void_p),
                ("lda", C.c_int32), ("ldb", C.c_int32), ("ldc", C.c_int32),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("n_out", C.c_int32), ("split_k", C.c_int32), ("accumulate", C.c_int32)]


# ---------------------------------------------------------------------------------------------------
# the plans, restated (csrc/hsad_gemm_plan.h): (k tiles per range, ranges, k tiles of the last range)
# ---------------------------------------------------------------------------------------------------
def plan_with_chunk(K, chunk):
    nk = K // TILE_K
    count = -(-nk // chunk)
    return chunk, count, nk - (count - 1) * chunk


def core_plan(K, split_k):
    """the grouped launch: an even number of k tiles per range, at least 2"""
    c = -(-(K // TILE_K) // split_k)
    c += c & 1
    return plan_with_chunk(K, max(c, 2))


def plain_plan(K, split_k):
    """gemm_launch's own split (hsad_gemm_nt_bf16_splitk): ceil(k tiles / split_k) per range"""
    return plan_with_chunk(K, -(-(K // TILE_K) // split_k))


def workspace_floats(shapes):
    """shapes: (M, N, K, split_k) per item -> floats hsad_gemm_group_workspace_floats asks for"""
    return sum(core_plan(K, s)[1] * M * N for M, N, K, s in shapes)


def work_items(shapes):
    """(tile, range) work items of the core launch per item (M a multiple of 256)"""
    return [(M // 256) * (-(-N // 256)) * core_plan(K, s)[1] for M, N, K, s in shapes]


def launch_grid(shapes, cus):
    items = sum(work_items(shapes))
    grid = min(items, cus)
    return grid & ~7 if grid >= 64 else grid


def tile_orders(shapes, cus):
    """g8_launch's rule: the tile order of every problem of a core launch on a chip of `cus` CUs"""
    grid, before, out = launch_grid(shapes, cus), 0, []
    for (M, N, K, s), n_items in zip(shapes, work_items(shapes)):
        tm, tn = M // 256, -(-N // 256)
        pn = 4 if tn % 4 == 0 else 2 if tn % 2 == 0 else 1
        xcd_ok = grid % 8 == 0 and before % 8 == 0
        order = 0
        if xcd_ok and tm % 8 == 0:
            order = 1
        if xcd_ok and (tm * tn) % 256 == 0 and tm % (32 // pn) == 0:
            order = 2
        out.append(order)
        before += n_items
    return out


# ---------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------
class Spec:
    """one problem: row_map None | "perm" (gate_block_perm(M / 4): a permutation of the M rows) | "scatter" (M distinct rows out of M + 3)"""

    def __init__(self, M, N, K, split_k, n_out=None, ldc=None, row_map=None, accumulate=0):
        self.M, self.N, self.K, self.split_k = M, N, K, split_k
        self.n_out = N if n_out is None else n_out
        self.ldc = self.n_out + 5 + (self.n_out & 1) if ldc is None else ldc      # odd, > n_out
        self.row_map, self.accumulate = row_map, accumulate

    @property
    def shape(self):
        return (self.M, self.N, self.K, self.split_k)

    def __repr__(self):
        return "Spec(M=%d N=%d K=%d split=%d n_out=%d ldc=%d map=%s acc=%d)" % (self.M, self.N, self.K, self.split_k, self.n_out, self.ldc,
                                                                             self.row_map, self.accumulate)


def _canary(n, salt):
    return ((torch.arange(n, dtype=torch.int64) * 2654435761 + salt) & 0xFFFF).to(torch.int32) | 0x4B1D0000


class Case:
    pass


def make_case(spec, seed, exact=True):
    M, N, K = spec.M, spec.N, spec.K
    g = torch.Generator(device="cpu").manual_seed(seed)
    c = Case()
    c.spec, c.exact = spec, exact
    if exact:
        A = torch.randint(-4, 5, (M, K), generator=g).to(torch.bfloat16)
        B = torch.randint(-4, 5, (N, K), generator=g).to(torch.bfloat16)
    else:
        A = (torch.randn(M, K, generator=g) * 0.5).to(torch.bfloat16)
        B = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    c.A, c.B = A, B
    # row map
    if spec.row_map == "perm":
        from hanabi_sad_amd.r2d2 import gate_block_perm
        c.map = gate_block_perm(M // 4, "cpu").to(torch.int64)
        assert sorted(c.map.tolist()) == list(range(M))
    elif spec.row_map == "scatter":
        c.map = torch.randperm(M + 3, generator=g)[:M]
    else:
        assert spec.row_map is None
        c.map = None
    rows_out = torch.arange(M) if c.map is None else c.map
    c.rows_out = rows_out
    c.rows_alloc = int(rows_out.max()) + 1 + 3
    ldc, n_out = spec.ldc, spec.n_out
    # C canvas: canary words everywhere, the payload pre-filled
    bits = _canary(c.rows_alloc * ldc, seed).view(c.rows_alloc, ldc)
    payload = torch.zeros(c.rows_alloc, ldc, dtype=torch.bool)
    if 0 < n_out <= ldc:
        payload[rows_out, :n_out] = True
    fill = torch.randint(-1024, 1025, (c.rows_alloc, ldc), generator=g).float() if spec.accumulate else torch.full((c.rows_alloc, ldc), float("nan"))
    c.C0 = torch.where(payload, fill.view(torch.int32), bits).view(torch.float32)
    c.payload = payload
    if exact:
        c0max = float(c.C0[payload].abs().max()) if spec.accumulate else 0.0
        assert float(A.float().abs().max()) * float(B.float().abs().max()) * K + c0max < 2 ** 24, "the case would rely on rounding"
    # device buffers with the poison
    c.lda, c.ldb = K + 8, K + 16
    Ad = torch.full((M + 8, c.lda), float("nan"), dtype=torch.bfloat16)
    Ad[:M, :K] = A
    Bd = torch.full((N + 8, c.ldb), float("nan"), dtype=torch.bfloat16)
    Bd[:N, :K] = B
    c.A_dev, c.B_dev = Ad.to(DEV), Bd.to(DEV)
    c.A_keep, c.B_keep = c.A_dev.clone(), c.B_dev.clone()
    c.C_dev = c.C0.to(DEV)
    c.map_dev = None if c.map is None else c.map.to(torch.int32).to(DEV)
    c._prod = None
    return c


def reset_case(c):
    c.C_dev.copy_(c.C0.to(DEV))


def product64(c):
    """fp64 A B^T on the CPU, once per case"""
    if c._prod is None:
        c._prod = c.A.double().numpy() @ c.B.double().numpy().T
    return c._prod


def abs_product64(c):
    return np.abs(c.A.double().numpy()) @ np.abs(c.B.double().numpy()).T


def reference(c, times=1):
    """the fp64 canvas the call must leave (payload only; NaN elsewhere): row_map, n_out, accumulate and ldc applied in numpy.
    times: the product is added that many times (repeated accumulating calls)"""
    s = c.spec
    want = np.full((c.rows_alloc, s.ldc), np.nan)
    rows = c.rows_out.numpy()
    base = c.C0.numpy().astype(np.float64)[rows, :s.n_out] if s.accumulate else 0.0
    want[rows, :s.n_out] = base + times * product64(c)[:, :s.n_out]
    return want


def item_of(c, A_off_bytes=0):
    s = c.spec
    return GroupItem(c.A_dev.data_ptr() + A_off_bytes, c.B_dev.data_ptr(), c.C_dev.data_ptr(), 0 if c.map_dev is None else c.map_dev.data_ptr(),
                     c.lda, c.ldb, s.ldc, s.M, s.N, s.K, s.n_out, s.split_k, s.accumulate)


# ---------------------------------------------------------------------------------------------------
# callers (prototypes: hanabi_sad_amd/_lib.py)
# ---------------------------------------------------------------------------------------------------
def _lib_and_stream():
    from hanabi_sad_amd import _lib
    from hanabi_sad_amd.r2d2 import _s
    return _lib.load_library(), _s(torch.device(DEV))


def item_array(items):
    return (GroupItem * len(items))(*items)


def group_workspace_floats(items):
    lib, _ = _lib_and_stream()
    arr = item_array(items)
    return int(lib.hsad_gemm_group_workspace_floats(len(items), C.cast(arr, C.c_void_p)))


class Workspace:
    """`floats` NaN floats and a tail of WS_TAIL pattern words behind them"""

    def __init__(self, floats):
        self.floats = floats
        self.tail0 = _canary(WS_TAIL, 77)
        self.buf = torch.empty(floats + WS_TAIL, dtype=torch.float32, device=DEV)
        self.poison()

    def poison(self):
        self.buf[:self.floats] = float("nan")
        self.buf[self.floats:] = self.tail0.view(torch.float32).to(DEV)

    def tail_intact(self):
        return torch.equal(self.buf[self.floats:].view(torch.int32).cpu(), self.tail0)

    def untouched(self):
        return self.tail_intact() and bool(torch.isnan(self.buf[:self.floats]).all())


def call_group(items, ws, workspace_floats_arg=None):
    """-> the entry point's return code (synchronised)"""
    lib, st = _lib_and_stream()
    arr = item_array(items)
    rc = lib.hsad_gemm_nt_bf16_group_splitk(len(items), C.cast(arr, C.c_void_p), ws.buf.data_ptr(),
                                            ws.floats if workspace_floats_arg is None else workspace_floats_arg, st)
    torch.cuda.synchronize()
    return rc


def call_splitk(c, ws, acc, A_off=0, B_off=0, K=None):
    """hsad_gemm_nt_bf16_splitk / _splitk_acc on case c (A_off / B_off in elements, K: a piece of the contraction)"""
    lib, st = _lib_and_stream()
    s = c.spec
    fn = lib.hsad_gemm_nt_bf16_splitk_acc if acc else lib.hsad_gemm_nt_bf16_splitk
    rc = fn(c.A_dev.data_ptr() + 2 * A_off, c.lda, c.B_dev.data_ptr() + 2 * B_off, c.ldb, s.M, s.N, s.K if K is None else K, s.split_k,
            ws.buf.data_ptr(), c.C_dev.data_ptr(), s.ldc, None if c.map_dev is None else c.map_dev.data_ptr(), st)
    torch.cuda.synchronize()
    return rc


# ---------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------
def operands_intact(c):
    return (torch.equal(c.A_dev.view(torch.int16), c.A_keep.view(torch.int16)) and
            torch.equal(c.B_dev.view(torch.int16), c.B_keep.view(torch.int16)))


def canvas_untouched(c):
    return torch.equal(c.C_dev.cpu().view(torch.int32), c.C0.view(torch.int32))


def check_canaries(c, got):
    """everything of the C canvas outside the payload is bitwise what it was, and so are the operands with their padding"""
    assert torch.equal(got.view(torch.int32)[~c.payload], c.C0.view(torch.int32)[~c.payload]), "%r: C was written outside n_out / row_map" % c.spec
    assert operands_intact(c), "%r: an operand buffer changed" % c.spec


def check_exact(c, times=1):
    """the whole payload EQUALS the fp64 product (a NaN anywhere fails), the canaries are intact"""
    assert c.exact
    got = c.C_dev.cpu()
    check_canaries(c, got)
    want = torch.from_numpy(reference(c, times)).float()
    g, w = got[c.payload], want[c.payload]
    assert torch.equal(g, w), "%r: %d of %d elements differ from the fp64 product (%d NaN), first at flat payload index %d" % (
        c.spec, int((g != w).sum()), g.numel(), int(torch.isnan(g).sum()), int((g != w).nonzero()[0]))


def rounded_error(c, nslab):
    """-> (max of |C - C64| / bound over the payload, where bound = (K + nslab) 2^-23 (|A| |B|^T) in fp64)"""
    s = c.spec
    got = c.C_dev.cpu()
    check_canaries(c, got)
    rows = c.rows_out.numpy()
    g = got.numpy().astype(np.float64)[rows, :s.n_out]
    assert not np.isnan(g).any(), "%r: NaN in the result" % c.spec
    err = np.abs(g - product64(c)[:, :s.n_out])
    bound = (s.K + nslab) * 2.0 ** -23 * abs_product64(c)[:, :s.n_out]
    assert (bound > 0).all()
    return float((err / bound).max())


def result_bits(c):
    return c.C_dev.cpu().view(torch.int32).clone()
