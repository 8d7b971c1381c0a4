"""HBM tuple batches and kernel launches.

torch is used only as the allocator of device memory and for streams/events (HIP under
ROCm); the compute is the C-ABI kernels. Tuples are SoA:
  src_ip u32, dst_ip u32, dport u16, proto u8 (+ sport u16 for connection mode).
"""
import ctypes as C

import numpy as np
import torch

from . import _capi
from ._capi import lib


class TupleBatch:
    def __init__(self, n, device="cuda", with_sport=True):
        self.n = n
        self.src = torch.empty(n, dtype=torch.int32, device=device)
        self.dst = torch.empty(n, dtype=torch.int32, device=device)
        self.dport = torch.empty(n, dtype=torch.int16, device=device)
        self.proto = torch.empty(n, dtype=torch.uint8, device=device)
        self.sport = torch.empty(n, dtype=torch.int16, device=device) if with_sport else None

    @classmethod
    def from_numpy(cls, src, dst, sport, dport, proto, device="cuda"):
        b = cls.__new__(cls)
        b.n = len(src)
        b.src = torch.from_numpy(np.ascontiguousarray(src, dtype=np.uint32).view(np.int32)).to(device)
        b.dst = torch.from_numpy(np.ascontiguousarray(dst, dtype=np.uint32).view(np.int32)).to(device)
        b.dport = torch.from_numpy(np.ascontiguousarray(dport, dtype=np.uint16).view(np.int16)).to(device)
        b.proto = torch.from_numpy(np.ascontiguousarray(proto, dtype=np.uint8)).to(device)
        b.sport = torch.from_numpy(np.ascontiguousarray(sport, dtype=np.uint16).view(np.int16)).to(device)
        return b

    def soa(self, offset=0):
        s = _capi.pg_tuple_soa()
        s.src_ip = self.src.data_ptr() + 4 * offset
        s.dst_ip = self.dst.data_ptr() + 4 * offset
        s.dst_port = self.dport.data_ptr() + 2 * offset
        s.proto = self.proto.data_ptr() + offset
        s.src_port = (self.sport.data_ptr() + 2 * offset) if self.sport is not None else None
        return s

    def numpy(self, k=None):
        k = self.n if k is None else k
        g = lambda t, dt: t[:k].cpu().numpy().view(dt)
        return (g(self.src, np.uint32), g(self.dst, np.uint32),
                g(self.sport, np.uint16) if self.sport is not None else np.zeros(k, np.uint16),
                g(self.dport, np.uint16), g(self.proto, np.uint8))


def _stream_ptr(stream):
    if stream is None:
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return C.c_void_p(stream.cuda_stream)


def gen_tuples(engine, batch, seed, table_id=-1, inside_pct=0, ip_pool=None, pool_pct=0, dst_pool_pct=0,
               port_pool=None, port_pool_pct=0, tcp_pct=45, udp_pct=45, zipf_cdf=None, nomatch_pct=0,
               index_base=0, stream=None):
    spec = _capi.pg_gen_spec()
    spec.seed, spec.index_base, spec.table_id, spec.inside_pct = seed, index_base, table_id, inside_pct
    keep = []
    if ip_pool is not None and len(ip_pool):
        a = np.ascontiguousarray(ip_pool, dtype=np.uint32)
        keep.append(a)
        spec.ip_pool = a.ctypes.data_as(C.POINTER(C.c_uint32))
        spec.n_ip_pool = len(a)
    if port_pool is not None and len(port_pool):
        p = np.ascontiguousarray(port_pool, dtype=np.uint16)
        keep.append(p)
        spec.port_pool = p.ctypes.data_as(C.POINTER(C.c_uint16))
        spec.n_port_pool = len(p)
    if zipf_cdf is not None:
        z = np.ascontiguousarray(zipf_cdf, dtype=np.uint32)
        keep.append(z)
        spec.zipf_cdf = z.ctypes.data_as(C.POINTER(C.c_uint32))
    spec.pool_pct, spec.dst_pool_pct, spec.port_pool_pct = pool_pct, dst_pool_pct, port_pool_pct
    spec.tcp_pct, spec.udp_pct, spec.nomatch_pct = tcp_pct, udp_pct, nomatch_pct
    sp = batch.sport.data_ptr() if batch.sport is not None else None
    engine._ck(lib.pg_gen_tuples(engine.h, C.byref(spec), batch.n, batch.src.data_ptr(), batch.dst.data_ptr(),
                                 sp, batch.dport.data_ptr(), batch.proto.data_ptr(), _stream_ptr(stream)))


def classify(engine, mode, table_id, batch, out, counters=None, stream=None, offset=0, n=None):
    n = batch.n - offset if n is None else n
    soa = batch.soa(offset)
    cptr = counters if (counters is None or isinstance(counters, int)) else counters.data_ptr()
    engine._ck(lib.pg_classify(engine.h, mode, table_id, C.byref(soa), n, out.data_ptr() + 4 * offset, cptr,
                               _stream_ptr(stream)))


def last_launch():
    """TESTS ONLY: {block, grid, resident} of this thread's last classify kernel launch
    (pg_debug_last_launch): threads per workgroup, workgroups launched, and the workgroups the
    device holds at once under the launch knobs"""
    b, g, r = C.c_int(), C.c_int(), C.c_int()
    if lib.pg_debug_last_launch(C.byref(b), C.byref(g), C.byref(r)) != 0:
        raise RuntimeError("pg_debug_last_launch")
    return {"block": b.value, "grid": g.value, "resident": r.value}


def classify_linear(engine, table_id, batch, out, stream=None):
    soa = batch.soa()
    engine._ck(lib.pg_classify_linear(engine.h, table_id, C.byref(soa), batch.n, out.data_ptr(),
                                      _stream_ptr(stream)))


def stream_probe(engine, fields, batch, out, stream=None):
    """pg_stream_probe: the loads and store of a classify launch over `batch` without the
    classification (fields: 1 = dst, 2 = sport) -- a measurement, not a classification"""
    soa = batch.soa()
    engine._ck(lib.pg_stream_probe(engine.h, fields, C.byref(soa), batch.n, out.data_ptr(), _stream_ptr(stream)))


def counters_device_ptr(engine):
    p = lib.pg_counters_device(engine.h)
    if not p:
        raise RuntimeError(lib.pg_last_error(engine.h).decode())
    return p


def read_counters(engine):
    n = engine.num_counter_slots()
    buf = (C.c_uint64 * n)()
    engine._ck(lib.pg_read_counters(engine.h, buf, n))
    return np.frombuffer(buf, dtype=np.uint64).copy()


def reset_counters(engine, stream=None):
    engine._ck(lib.pg_reset_counters(engine.h, _stream_ptr(stream)))


def counters_snapshot(engine):
    """the gauge snapshot (pg_counters_snapshot: the cluster sum once a communicator exists,
    else this GPU's counts as of the last read; no GPU access)"""
    n = engine._ck(lib.pg_counters_snapshot(engine.h, None, 0))
    buf = (C.c_uint64 * max(1, n))()
    engine._ck(lib.pg_counters_snapshot(engine.h, buf, n))
    return np.frombuffer(buf, dtype=np.uint64)[:n].copy()


def counters_snapshot_range(engine, which, first, n):
    """slots [first, first + n) of a host snapshot (SNAP_LOCAL / SNAP_CLUSTER / SNAP_GAUGE)
    -> (u64 array, its layout generation); no GPU access"""
    buf = (C.c_uint64 * max(1, n))()
    gen = C.c_uint64()
    k = engine._ck(lib.pg_counters_snapshot_range(engine.h, which, first, n, buf, C.byref(gen)))
    return np.frombuffer(buf, dtype=np.uint64)[:k].copy(), gen.value


def counter_of_rule(engine, which, acl_name, rule_index):
    """one rule's count in a host snapshot by (ACL name, rule index; -1 = default deny; name
    None: -1 "no ACL", -2 unresolved) resolved in that snapshot's layout -> (value, layout
    generation), or None when the snapshot has no such rule; no GPU access"""
    v, gen = C.c_uint64(), C.c_uint64()
    rc = lib.pg_counter_of_rule(engine.h, which, acl_name.encode() if acl_name is not None else None, rule_index,
                                C.byref(v), C.byref(gen))
    if rc == _capi.PG_ENOENT:
        return None
    engine._ck(rc)
    return v.value, gen.value


def counter_layout_gen(engine):
    return lib.pg_counter_layout_gen(engine.h)


# ---- RCCL counter all-reduce through the C ABI (include/policygpu.h pg_comm_*) -------------
def comm_unique_id():
    buf = C.create_string_buffer(128)
    rc = lib.pg_comm_unique_id(buf)
    if rc < 0:
        raise RuntimeError("pg_comm_unique_id failed (%d)" % rc)
    return buf.raw


def comm_init_rank(engine, nranks, uid, rank):
    engine._ck(lib.pg_comm_init_rank(engine.h, nranks, C.create_string_buffer(uid, 128), rank))


def comm_init_all(engines):
    arr = (C.c_void_p * len(engines))(*[e.h for e in engines])
    rc = lib.pg_comm_init_all(arr, len(engines))
    if rc < 0:
        engines[0]._ck(rc)


def allreduce_counters(engine, stream=None):
    """sum this rank's device counters over the communicator -> the summed counters (the
    device counters themselves keep this rank's counts)"""
    engine._ck(lib.pg_allreduce_counters(engine.h, _stream_ptr(stream)))
    return counters_snapshot(engine)


def allreduce_counters_all(engines):
    arr = (C.c_void_p * len(engines))(*[e.h for e in engines])
    rc = lib.pg_allreduce_counters_all(arr, len(engines))
    if rc < 0:
        for e in engines:
            msg = lib.pg_last_error(e.h).decode()
            if msg:
                raise RuntimeError("%s (code %d)" % (msg, rc))
        raise RuntimeError("pg_allreduce_counters_all failed (%d)" % rc)
    return [counters_snapshot(e) for e in engines]


# ---- reachability matrix (include/policygpu.h pg_reach_matrix) -------------------------------
def reach_spec(src_ips, dst_ips, services):
    """pg_reach_spec over host arrays: IPv4 addresses as u32, services as (protocol, src port, dst
    port) -> (spec, the arrays it points into: keep them alive for the call)"""
    src = np.ascontiguousarray(src_ips, dtype=np.uint32)
    dst = np.ascontiguousarray(dst_ips, dtype=np.uint32)
    svc = (_capi.pg_service * max(1, len(services)))()
    for i, (proto, sport, dport) in enumerate(services):
        svc[i].protocol, svc[i].src_port, svc[i].dst_port = int(proto), int(sport), int(dport)
    spec = _capi.pg_reach_spec(src.ctypes.data, len(src), dst.ctypes.data, len(dst), svc, len(services))
    return spec, (src, dst, svc)


def reach_row_words(n_dst):
    return lib.pg_reach_row_words(n_dst)


def reach_matrix(engine, src_ips, dst_ips, services, words=False, stream=None):
    """testConnection of every (service, src, dst) on the GPU (pg_reach_matrix) -> the packed
    ConnActions, an int32 tensor [n_svc, n_src, row_words] (2 bits per pair, unpack_reach), and with
    ``words`` also the full verdict words, an int32 tensor [n_svc, n_src, n_dst]. The call never
    touches the hit counters."""
    spec, keep = reach_spec(src_ips, dst_ips, services)
    n_svc, n_src, n_dst = len(services), spec.n_src, spec.n_dst
    packed = torch.empty((n_svc, n_src, reach_row_words(n_dst)), dtype=torch.int32, device="cuda")
    full = torch.empty((n_svc, n_src, n_dst), dtype=torch.int32, device="cuda") if words else None
    if packed.numel() == 0:  # (an empty tensor has no address to hand over; the call would write nothing)
        return (packed, full) if words else packed
    engine._ck(lib.pg_reach_matrix(engine.h, C.byref(spec), packed.data_ptr(), full.data_ptr() if words else None,
                                   _stream_ptr(stream)))
    del keep
    return (packed, full) if words else packed


def unpack_reach(packed, n_svc, n_src, n_dst):
    """packed reachability words (tensor or array) -> uint8 ConnActions [n_svc, n_src, n_dst]"""
    if isinstance(packed, torch.Tensor):
        packed = packed.cpu().numpy()
    w = np.ascontiguousarray(packed).view(np.uint32).reshape(n_svc, n_src, reach_row_words(n_dst))
    codes = (w[..., None] >> (2 * np.arange(16, dtype=np.uint32))) & 3
    return codes.reshape(n_svc, n_src, 16 * w.shape[2])[..., :n_dst].astype(np.uint8)


# ---- port sweep (include/policygpu.h pg_reach_ports) ------------------------------------------
def port_intervals(engine, protocol):
    """the lower bounds of the elementary dst-port intervals of TCP (0) or UDP (1) over the
    installed ACLs (pg_port_intervals): a uint32 array lo[K], lo[0] = 0, ascending; interval k ends
    at lo[k + 1] - 1, the last at 65535"""
    k = engine._ck(lib.pg_port_intervals(engine.h, int(protocol), None, 0))
    lo = np.empty(k, np.uint32)
    engine._ck(lib.pg_port_intervals(engine.h, int(protocol), lo.ctypes.data_as(C.c_void_p), k))
    return lo


def ports_spec(src_ips, dst_ips, protocol, src_port, n_intervals):
    """pg_port_sweep_spec over host arrays -> (spec, the arrays it points into: keep them alive)"""
    src = np.ascontiguousarray(src_ips, dtype=np.uint32)
    dst = np.ascontiguousarray(dst_ips, dtype=np.uint32)
    spec = _capi.pg_port_sweep_spec(src.ctypes.data, len(src), dst.ctypes.data, len(dst), int(protocol),
                                    int(src_port), 0, int(n_intervals))
    return spec, (src, dst)


def reach_ports(engine, src_ips, dst_ips, protocol, src_port=40000, open_count=False, words=False, stream=None):
    """testConnection of every (src, dst) on every dst port of TCP / UDP on the GPU (pg_reach_ports),
    one evaluation per elementary port interval -> (lo, codes[, open][, words]): the interval bounds
    (port_intervals), the packed ConnActions as an int32 tensor [n_src, n_dst, row_words(K)] (2 bits
    per interval, unpack_ports), with ``open_count`` the open (ALLOW) ports per pair, int32 [n_src,
    n_dst], and with ``words`` the full verdict words, int32 [n_src, n_dst, K]. The call never
    touches the hit counters."""
    lo = port_intervals(engine, protocol)
    k = len(lo)
    spec, keep = ports_spec(src_ips, dst_ips, protocol, src_port, k)
    n_src, n_dst = spec.n_src, spec.n_dst
    codes = torch.empty((n_src, n_dst, reach_row_words(k)), dtype=torch.int32, device="cuda")
    n_open = torch.empty((n_src, n_dst), dtype=torch.int32, device="cuda") if open_count else None
    full = torch.empty((n_src, n_dst, k), dtype=torch.int32, device="cuda") if words else None
    if codes.numel():  # (an empty tensor has no address to hand over; the call would write nothing)
        engine._ck(lib.pg_reach_ports(engine.h, C.byref(spec), codes.data_ptr(),
                                      n_open.data_ptr() if open_count else None,
                                      full.data_ptr() if words else None, _stream_ptr(stream)))
    del keep
    return (lo, codes) + ((n_open,) if open_count else ()) + ((full,) if words else ())


def unpack_ports(codes, n_src, n_dst, k):
    """packed sweep codes (tensor or array) -> uint8 ConnActions [n_src, n_dst, K]"""
    return unpack_reach(codes, n_src, n_dst, k)


# ---- reachability diff (include/policygpu.h pg_reach_diff) -----------------------------------
DIFF_ALL, DIFF_OPENED, DIFF_CLOSED = _capi.DIFF_ALL, _capi.DIFF_OPENED, _capi.DIFF_CLOSED


def reach_diff(engine, before, after, n_cols, transitions=DIFF_ALL, cap=None, row_changes=False, stream=None):
    """The cells in which two packed audit results differ, on the GPU (pg_reach_diff). ``before`` and
    ``after`` are int32 device tensors of one shape [..., row_words(n_cols)]: two reach_matrix results
    (n_cols = n_dst) or two reach_ports code tensors over one partition (n_cols = K); rows are the
    leading dimensions flattened. -> (n_changes, changes, trans, row_changes): the number of selected
    cells, the first min(n_changes, cap) of them in (row, column) order as an int32 tensor [m, 2]
    (unpack_changes), the uint64 array trans[before, after] over all cells, and with ``row_changes``
    an int32 tensor [n_rows], else None. ``cap`` None: a count-only call first, then one sized
    exactly; 0: count only. The call never touches the hit counters."""
    rw = reach_row_words(n_cols)
    if before.shape != after.shape or before.dtype != torch.int32 or after.dtype != torch.int32:
        raise ValueError("before and after must be int32 tensors of one shape")
    if not (before.is_contiguous() and after.is_contiguous()) or (before.numel() and before.shape[-1] != rw):
        raise ValueError("contiguous tensors [..., row_words(n_cols)] expected")
    n_rows = before.numel() // rw
    rows = torch.empty(n_rows, dtype=torch.int32, device="cuda") if row_changes else None
    trans = np.zeros(16, np.uint64)
    if n_rows == 0:  # (an empty tensor has no address to hand over; the call would write nothing)
        return 0, torch.empty((0, 2), dtype=torch.int32, device="cuda"), trans.reshape(4, 4), rows

    def call(changes, cap, rows, want_trans):
        spec = _capi.pg_reach_diff_spec(before.data_ptr(), after.data_ptr(), n_rows, int(n_cols), int(transitions), cap)
        n = C.c_uint64()
        engine._ck(lib.pg_reach_diff(engine.h, C.byref(spec), changes.data_ptr() if cap else None,
                                     rows.data_ptr() if rows is not None else None, C.byref(n),
                                     trans.ctypes.data_as(C.c_void_p) if want_trans else None, _stream_ptr(stream)))
        return n.value

    if cap is None:
        cap = call(None, 0, None, False)
    changes = torch.empty((cap, 2), dtype=torch.int32, device="cuda")
    n = call(changes, cap, rows, True)
    return n, changes[:min(n, cap)], trans.reshape(4, 4), rows


def unpack_changes(changes):
    """pg_reach_change entries (tensor or array [m, 2]) -> (row, column, ConnAction before, after)
    arrays"""
    if isinstance(changes, torch.Tensor):
        changes = changes.cpu().numpy()
    c = np.ascontiguousarray(changes).view(np.uint32).reshape(-1, 2)
    cell = c[:, 1]
    return c[:, 0].copy(), cell & 0xFFFFF, ((cell >> 28) & 3).astype(np.uint8), (cell >> 30).astype(np.uint8)


# ---- reachability closure (include/policygpu.h pg_reach_closure) ----------------------------
def closure_spec(matrix_ptr, n, n_svc, svc_select=None, max_hops=0):
    """pg_reach_closure_spec -> (spec, the array it points into: keep it alive for the call)"""
    sel = None
    if svc_select is not None:
        sel = np.ascontiguousarray(np.asarray(svc_select) != 0, dtype=np.uint8)
        if sel.shape != (n_svc,):
            raise ValueError("svc_select takes one entry per slice")
    spec = _capi.pg_reach_closure_spec(matrix_ptr, int(n), int(n_svc), sel.ctypes.data if sel is not None else None,
                                       int(max_hops))
    return spec, sel


def closure_result(res):
    return {"levels": res.levels, "n_edges": res.n_edges, "n_reachable": res.n_reachable}


def reach_closure(engine, matrix, n, svc_select=None, max_hops=0, hops=False, counts=False, stream=None):
    """Multi-hop reach over the ALLOW graph of a square reach_matrix result, on the GPU
    (pg_reach_closure). ``matrix`` is an int32 device tensor [n_svc, n, row_words(n)] taken with one
    end-point list on both sides; ``svc_select`` (one flag per slice, None = all) says which slices
    contribute edges; ``max_hops`` 0 = until nothing new is found. -> (packed, hops, counts, result):
    the closure as an int32 tensor [n, row_words(n)] in the audits' layout (ALLOW = reachable;
    unpack_closure, or reach_diff over two of them), with ``hops`` the hop counts as an int16 tensor
    [n, n] (0 = not reachable) else None, with ``counts`` the reachable cells of every row as an int32
    tensor [n] else None, and {levels, n_edges, n_reachable}. The call never touches the hit
    counters."""
    rw = reach_row_words(n)
    if matrix.dtype != torch.int32 or not matrix.is_contiguous() or matrix.numel() % max(1, n * rw):
        raise ValueError("a contiguous int32 tensor [n_svc, n, row_words(n)] expected")
    n_svc = matrix.numel() // max(1, n * rw)
    packed = torch.empty((n, rw), dtype=torch.int32, device="cuda")
    hop = torch.empty((n, n), dtype=torch.int16, device="cuda") if hops else None
    cnt = torch.empty(n, dtype=torch.int32, device="cuda") if counts else None
    res = _capi.pg_reach_closure_result()
    if n == 0:  # (an empty tensor has no address to hand over; the call would write nothing)
        return packed, hop, cnt, closure_result(res)
    spec, keep = closure_spec(matrix.data_ptr(), n, n_svc, svc_select, max_hops)
    engine._ck(lib.pg_reach_closure(engine.h, C.byref(spec), packed.data_ptr(), hop.data_ptr() if hops else None,
                                    cnt.data_ptr() if counts else None, C.byref(res), _stream_ptr(stream)))
    del keep
    return packed, hop, cnt, closure_result(res)


def unpack_closure(packed, n):
    """packed closure words (tensor or array [n, row_words(n)]) -> bool [n, n], True = reachable"""
    return unpack_reach(packed, 1, n, n)[0] == 2   # PG_CONN_ALLOW


# ---- reachability groups (include/policygpu.h pg_reach_groups) -------------------------------
GROUP_SKIP = _capi.GROUP_SKIP


def groups_spec(matrix_ptr, n_svc, n_src, n_dst, src_group, dst_group, n_src_groups, n_dst_groups):
    """pg_reach_groups_spec -> (spec, the arrays it points into: keep them alive for the call)"""
    sg = np.ascontiguousarray(src_group, dtype=np.uint32)
    dg = np.ascontiguousarray(dst_group, dtype=np.uint32)
    if sg.shape != (n_src,) or dg.shape != (n_dst,):
        raise ValueError("src_group / dst_group take one id per end point")
    spec = _capi.pg_reach_groups_spec(matrix_ptr, int(n_svc), int(n_src), int(n_dst), sg.ctypes.data if n_src else None,
                                      dg.ctypes.data if n_dst else None, int(n_src_groups), int(n_dst_groups))
    return spec, (sg, dg)


def reach_groups(engine, matrix, n_src, n_dst, src_group, dst_group, n_src_groups, n_dst_groups, packed=False,
                 stream=None):
    """A reach_matrix result summed into (src group, dst group) pairs, on the GPU (pg_reach_groups).
    ``matrix`` is an int32 device tensor [n_svc, n_src, row_words(n_dst)]; ``src_group`` / ``dst_group``
    give every end point a group id below its count, or GROUP_SKIP. -> (counts, packed): the cells of
    every (service, src group, dst group) by ConnAction as an int64 tensor [n_svc, n_sg, n_dg, 4], and
    with ``packed`` the GROUPS_* status of every pair as an int32 tensor [n_svc, n_sg, row_words(n_dg)]
    in the audits' layout (unpack_groups, or reach_diff over two of them with n_cols = n_dg), else
    None. The call never touches the hit counters."""
    rw = reach_row_words(n_dst)
    if matrix.dtype != torch.int32 or not matrix.is_contiguous() or matrix.numel() % max(1, n_src * rw):
        raise ValueError("a contiguous int32 tensor [n_svc, n_src, row_words(n_dst)] expected")
    n_svc = matrix.shape[0] if matrix.dim() == 3 else matrix.numel() // max(1, n_src * rw)
    counts = torch.empty((n_svc, n_src_groups, n_dst_groups, 4), dtype=torch.int64, device="cuda")
    status = torch.empty((n_svc, n_src_groups, reach_row_words(n_dst_groups)), dtype=torch.int32,
                         device="cuda") if packed else None
    if counts.numel() == 0:  # (an empty tensor has no address to hand over; the call would write nothing)
        return counts, status
    spec, keep = groups_spec(matrix.data_ptr() if matrix.numel() else None, n_svc, n_src, n_dst, src_group, dst_group,
                             n_src_groups, n_dst_groups)
    engine._ck(lib.pg_reach_groups(engine.h, C.byref(spec), counts.data_ptr(), status.data_ptr() if packed else None,
                                   _stream_ptr(stream)))
    del keep
    return counts, status


def unpack_groups(packed, n_dst_groups):
    """packed group status words (tensor or array [..., row_words(n_dst_groups)]) -> uint8 GROUPS_*
    [..., n_dst_groups]"""
    if isinstance(packed, torch.Tensor):
        packed = packed.cpu().numpy()
    w = np.ascontiguousarray(packed).view(np.uint32)
    return unpack_reach(w, 1, w.size // max(1, w.shape[-1]), n_dst_groups).reshape(w.shape[:-1] + (n_dst_groups,))


# ---- reachability paths (include/policygpu.h pg_reach_paths) ---------------------------------
PATHS_NONE = 0xFFFF   # a nodes entry behind the path; every entry of a row without one


def paths_spec(hops_ptr, n, src, dst, max_len):
    """pg_reach_paths_spec -> (spec, the arrays it points into: keep them alive for the call)"""
    s = np.ascontiguousarray(src, dtype=np.uint32)
    d = np.ascontiguousarray(dst, dtype=np.uint32)
    if s.ndim != 1 or s.shape != d.shape:
        raise ValueError("src and dst take one id per query")
    spec = _capi.pg_reach_paths_spec(hops_ptr, int(n), s.ctypes.data if s.size else None, d.ctypes.data if s.size else None,
                                     s.size, int(max_len))
    return spec, (s, d)


def paths_result(res):
    return {"n_found": res.n_found, "n_unreachable": res.n_unreachable, "n_too_long": res.n_too_long,
            "n_broken": res.n_broken, "n_via": res.n_via, "longest": res.longest}


def reach_paths(engine, hops, n, src, dst, max_len=None, nodes=True, via=False, stream=None):
    """One shortest path per (src, dst) query over a reach_closure ``hops`` tensor (int16 [n, n], on the
    device), and the choke points, on the GPU (pg_reach_paths). The path of a query is the one the
    least-predecessor rule of include/policygpu.h defines. -> (lengths, nodes, via, result): the edges
    of every path as an int16 tensor [n_queries] (0 = unreachable or broken), with ``nodes`` the paths
    as an int16 tensor [n_queries, max_len + 1] (p_0 .. p_d, then PATHS_NONE; unpack_paths) else None,
    with ``via`` the number of paths that pass through every end point as an int32 tensor [n] else
    None, and {n_found, n_unreachable, n_too_long, n_broken, n_via, longest}. ``max_len`` None: n, which
    no shortest path exceeds. The call never touches the hit counters."""
    if hops.dtype != torch.int16 or not hops.is_contiguous() or hops.numel() != n * n:
        raise ValueError("a contiguous int16 tensor [n, n] expected")
    max_len = max(1, n) if max_len is None else int(max_len)
    spec, keep = paths_spec(hops.data_ptr(), n, src, dst, max_len)
    nq = int(spec.n_queries)
    lens = torch.empty(nq, dtype=torch.int16, device="cuda")
    rows = torch.empty((nq, max_len + 1), dtype=torch.int16, device="cuda") if nodes else None
    cnt = torch.empty(n, dtype=torch.int32, device="cuda") if via else None
    res = _capi.pg_reach_paths_result()
    if n == 0 or (nq == 0 and not via):  # (an empty tensor has no address to hand over; the call would write nothing)
        return lens, rows, cnt, paths_result(res)
    # (without a query out_len has no entry: any address that is not null will do)
    engine._ck(lib.pg_reach_paths(engine.h, C.byref(spec), lens.data_ptr() if nq else hops.data_ptr(),
                                  rows.data_ptr() if nodes and nq else None, cnt.data_ptr() if via else None,
                                  C.byref(res), _stream_ptr(stream)))
    del keep
    return lens, rows, cnt, paths_result(res)


def unpack_paths(lengths, nodes):
    """path lengths [n_queries] and nodes rows [n_queries, max_len + 1] (tensors or arrays) -> one list of
    node indices per query, None where the query has no path or the path is too long for its row"""
    if isinstance(lengths, torch.Tensor):
        lengths = lengths.cpu().numpy()
    if isinstance(nodes, torch.Tensor):
        nodes = nodes.cpu().numpy()
    d = np.ascontiguousarray(lengths).view(np.uint16)
    rows = np.ascontiguousarray(nodes).view(np.uint16)
    return [rows[q, :int(d[q]) + 1].tolist() if d[q] and d[q] < rows.shape[1] and rows[q, 0] != PATHS_NONE else None
            for q in range(d.size)]


# ---- reachability classes (include/policygpu.h pg_reach_classes) -----------------------------
def classes_result(res):
    return {"n_src_classes": res.n_src_classes, "n_dst_classes": res.n_dst_classes, "rounds": res.rounds}


def reach_classes(engine, matrix, n_svc, n_src, n_dst, src=True, dst=True, reps=False, quotient=False, stream=None):
    """The end points of a reach_matrix result that the policy treats identically, on the GPU
    (pg_reach_classes). ``matrix`` is an int32 device tensor [n_svc, n_src, row_words(n_dst)]; ``src`` /
    ``dst`` say which sides are classed. -> (src_class, dst_class, src_rep, dst_rep, quotient, result):
    the class of every end point as int32 tensors [n_src] / [n_dst], numbered by first appearance; with
    ``reps`` each class's least member as int32 tensors [n_src_classes] / [n_dst_classes]; with
    ``quotient`` (both sides) the matrix of the representatives as an int32 tensor [n_svc,
    n_src_classes, row_words(n_dst_classes)] in the audits' layout (unpack_reach, reach_diff,
    reach_groups); and {n_src_classes, n_dst_classes, rounds}. Whatever was not asked for is None. The
    call never touches the hit counters."""
    rw = reach_row_words(n_dst)
    if matrix.dtype != torch.int32 or not matrix.is_contiguous() or matrix.numel() != n_svc * n_src * rw:
        raise ValueError("a contiguous int32 tensor [n_svc, n_src, row_words(n_dst)] expected")
    if not (src or dst) or (quotient and not (src and dst)):
        raise ValueError("at least one side, and both for the quotient")
    new = lambda n: torch.empty(n, dtype=torch.int32, device="cuda")
    sc, dc = new(n_src) if src else None, new(n_dst) if dst else None
    sr, dr = new(n_src) if src and reps else None, new(n_dst) if dst and reps else None
    q = new(matrix.numel()) if quotient else None
    res = _capi.pg_reach_classes_result()
    if matrix.numel():  # (an empty tensor has no address to hand over; the call would write nothing)
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        engine._ck(lib.pg_reach_classes(engine.h, C.byref(_capi.pg_reach_classes_spec(matrix.data_ptr(), int(n_svc), int(n_src),
                                                                                      int(n_dst))),
                                        ptr(sc), ptr(dc), ptr(sr), ptr(dr), ptr(q), C.byref(res), _stream_ptr(stream)))
    n_sc, n_dc = res.n_src_classes, res.n_dst_classes
    if sr is not None:
        sr = sr[:n_sc]
    if dr is not None:
        dr = dr[:n_dc]
    if q is not None:
        q = q[:n_svc * n_sc * reach_row_words(n_dc)].reshape(n_svc, n_sc, reach_row_words(n_dc))
    return sc, dc, sr, dr, q, classes_result(res)


# ---- reachability zones (include/policygpu.h pg_reach_zones) ---------------------------------
def zones_result(res):
    return {"n_zones": res.n_zones, "n_cyclic": res.n_cyclic, "n_multi": res.n_multi, "largest": res.largest,
            "n_broken": res.n_broken}


def reach_zones(engine, closure, n, reps=False, sizes=False, counts=False, dag=False, stream=None):
    """The end points of a reach_closure result that can all reach each other, and the graph of those
    zones, on the GPU (pg_reach_zones). ``closure`` is an int32 device tensor [n, row_words(n)] in the
    audits' layout (reach_closure's packed result; any matrix of that shape is defined). -> (zone, rep,
    size, reaches, reached_by, dag, result): the zone of every end point as an int32 tensor [n], numbered
    by first appearance; with ``reps`` each zone's least member and with ``sizes`` its members, int32
    tensors [n_zones]; with ``counts`` the end points each zone reaches and is reached by, two int32
    tensors [n_zones]; with ``dag`` (it takes the representatives: they are returned too) the zone graph
    as an int32 tensor [n_zones, row_words(n_zones)] in the audits' layout (unpack_closure, reach_diff);
    and {n_zones, n_cyclic, n_multi, largest, n_broken}. Whatever was not asked for is None. The call
    never touches the hit counters."""
    rw = reach_row_words(n)
    if closure.dtype != torch.int32 or not closure.is_contiguous() or closure.numel() != n * rw:
        raise ValueError("a contiguous int32 tensor [n, row_words(n)] expected")
    reps = reps or dag
    new = lambda k: torch.empty(k, dtype=torch.int32, device="cuda")
    zone = new(n)
    rep, size = new(n) if reps else None, new(n) if sizes else None
    out, by = (new(n), new(n)) if counts else (None, None)
    graph = new(n * rw) if dag else None
    res = _capi.pg_reach_zones_result()
    if n:  # (an empty tensor has no address to hand over; the call would write nothing)
        ptr = lambda t: t.data_ptr() if t is not None else None
        engine._ck(lib.pg_reach_zones(engine.h, C.byref(_capi.pg_reach_zones_spec(closure.data_ptr(), int(n))), ptr(zone),
                                      ptr(rep), ptr(size), ptr(out), ptr(by), ptr(graph), C.byref(res), _stream_ptr(stream)))
    nz = res.n_zones
    cut = lambda t: None if t is None else t[:nz]
    if graph is not None:
        graph = graph[:nz * reach_row_words(nz)].reshape(nz, reach_row_words(nz))
    return zone, cut(rep), cut(size), cut(out), cut(by), graph, zones_result(res)


# ---- reachability dominators (include/policygpu.h pg_reach_dominators) -----------------------
NO_IDOM = 0xFFFF


def dominators_spec(matrix_ptr, n, n_svc, entry, svc_select=None):
    """pg_reach_dominators_spec -> (spec, the arrays it points into: keep them alive for the call)"""
    sel = None
    if svc_select is not None:
        sel = np.ascontiguousarray(np.asarray(svc_select) != 0, dtype=np.uint8)
        if sel.shape != (n_svc,):
            raise ValueError("svc_select takes one entry per slice")
    ent = np.ascontiguousarray(entry, dtype=np.uint32).reshape(-1)
    spec = _capi.pg_reach_dominators_spec(matrix_ptr, int(n), int(n_svc), sel.ctypes.data if sel is not None else None,
                                          ent.ctypes.data if len(ent) else None, len(ent))
    return spec, (sel, ent)


def dominators_result(res):
    return {"n_reached": res.n_reached, "n_chokes": res.n_chokes, "top": res.top, "top_cut": res.top_cut,
            "depth": res.depth, "rounds": res.rounds}


def reach_dominators(engine, matrix, n, n_svc, entry, svc_select=None, dom=False, idom=False, cut=False, stream=None):
    """The end points every walk from the entry set must cross, over the ALLOW graph of a square
    reach_matrix result, on the GPU (pg_reach_dominators). ``matrix`` is an int32 device tensor [n_svc, n,
    row_words(n)] taken with one end-point list on both sides; ``entry`` the ids of the foothold
    (duplicates allowed); ``svc_select`` (one flag per slice, None = all) says which slices contribute
    edges. -> (dom, idom, cut, result): with ``dom`` the dominator sets as an int32 tensor [n,
    row_words(n)] in the audits' layout (cell (v, k) ALLOW = k dominates v; unpack_closure, reach_diff,
    reach_groups), with ``idom`` the immediate dominators as an int16 tensor [n] (view it as uint16:
    NO_IDOM where there is none), with ``cut`` the end points lost with each end point as an int32
    tensor [n], and {n_reached, n_chokes, top, top_cut, depth, rounds}. Whatever was not asked for is
    None. The call never touches the hit counters."""
    rw = reach_row_words(n)
    if matrix.dtype != torch.int32 or not matrix.is_contiguous() or matrix.numel() != n_svc * n * rw:
        raise ValueError("a contiguous int32 tensor [n_svc, n, row_words(n)] expected")
    d = torch.empty((n, rw), dtype=torch.int32, device="cuda") if dom else None
    i = torch.empty(n, dtype=torch.int16, device="cuda") if idom else None
    c = torch.empty(n, dtype=torch.int32, device="cuda") if cut else None
    res = _capi.pg_reach_dominators_result()
    spec, keep = dominators_spec(matrix.data_ptr() if n else None, n, n_svc, entry, svc_select)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    engine._ck(lib.pg_reach_dominators(engine.h, C.byref(spec), ptr(d), ptr(i), ptr(c), C.byref(res), _stream_ptr(stream)))
    del keep
    return d, i, c, dominators_result(res)


# ---- reachability cut (include/policygpu.h pg_reach_cut) --------------------------------------
NO_HOP = 0xFFFF
NO_CUT = 0xFFFFFFFF


def cut_spec(matrix_ptr, n, n_svc, entry, target, max_cut=16, svc_select=None):
    """pg_reach_cut_spec -> (spec, the arrays it points into: keep them alive for the call)"""
    sel = None
    if svc_select is not None:
        sel = np.ascontiguousarray(np.asarray(svc_select) != 0, dtype=np.uint8)
        if sel.shape != (n_svc,):
            raise ValueError("svc_select takes one entry per slice")
    ent = np.ascontiguousarray(entry, dtype=np.uint32).reshape(-1)
    tgt = np.ascontiguousarray(target, dtype=np.uint32).reshape(-1)
    spec = _capi.pg_reach_cut_spec(matrix_ptr, int(n), int(n_svc), sel.ctypes.data if sel is not None else None,
                                   ent.ctypes.data if len(ent) else None, len(ent),
                                   tgt.ctypes.data if len(tgt) else None, len(tgt), int(max_cut))
    return spec, (sel, ent, tgt)


def cut_result(res):
    return {name: getattr(res, name) for name, _ in res._fields_}


def reach_cut(engine, matrix, n, n_svc, entry, target, max_cut=16, svc_select=None, cut=False, paths=False, stream=None):
    """The fewest end points outside ``entry`` and ``target`` whose removal leaves no walk from an entry to
    a target, over the ALLOW graph of a square reach_matrix result, on the GPU (pg_reach_cut). ``matrix`` is
    an int32 device tensor [n_svc, n, row_words(n)] taken with one end-point list on both sides; ``entry``
    and ``target`` are ids (duplicates allowed); ``svc_select`` (one flag per slice, None = all) says which
    slices contribute edges; the search stops at ``max_cut`` + 1 disjoint paths. -> (cut, prev, next,
    result): with ``cut`` the flags as a uint8 tensor [n] (_capi.CUT_NEAR, CUT_FAR, CUT_NEAR_REACH,
    CUT_FAR_REACH), with ``paths`` the witness paths as two int16 tensors [n] (view them as uint16: NO_HOP
    off the paths), and {separable, capped, n_direct, cut_size, n_paths, near_reach, far_reach, levels,
    reroutes} (cut_size NO_CUT when there is none to report). Whatever was not asked for is None. The call
    never touches the hit counters."""
    rw = reach_row_words(n)
    if matrix.dtype != torch.int32 or not matrix.is_contiguous() or matrix.numel() != n_svc * n * rw:
        raise ValueError("a contiguous int32 tensor [n_svc, n, row_words(n)] expected")
    c = torch.empty(n, dtype=torch.uint8, device="cuda") if cut else None
    pv = torch.empty(n, dtype=torch.int16, device="cuda") if paths else None
    nx = torch.empty(n, dtype=torch.int16, device="cuda") if paths else None
    res = _capi.pg_reach_cut_result()
    spec, keep = cut_spec(matrix.data_ptr() if n else None, n, n_svc, entry, target, max_cut, svc_select)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    engine._ck(lib.pg_reach_cut(engine.h, C.byref(spec), ptr(c), ptr(pv), ptr(nx), C.byref(res), _stream_ptr(stream)))
    del keep
    return c, pv, nx, cut_result(res)


def cut_routes(prev, nxt, entries):
    """the witness paths of a reach_cut as lists of ids, entry first, target last, by their first interior
    end point ascending; prev / nxt are uint16 host arrays"""
    held = set(int(e) for e in entries)
    routes = []
    for v in range(len(prev)):
        if prev[v] != NO_HOP and int(prev[v]) in held:
            route = [int(prev[v]), v]
            while nxt[route[-1]] != NO_HOP and len(route) <= len(prev) + 1:
                route.append(int(nxt[route[-1]]))
            routes.append(route)
    return routes


# ---- reachability cost (include/policygpu.h pg_reach_cost) ------------------------------------
NO_COST = _capi.NO_COST
NO_PRED = _capi.NO_PRED


def cost_spec(matrix_ptr, n, n_svc, src, weight, max_cost=0, svc_select=None):
    """pg_reach_cost_spec -> (spec, the arrays it points into: keep them alive for the call)"""
    sel = None
    if svc_select is not None:
        sel = np.ascontiguousarray(np.asarray(svc_select) != 0, dtype=np.uint8)
        if sel.shape != (n_svc,):
            raise ValueError("svc_select takes one entry per slice")
    s = np.ascontiguousarray(src, dtype=np.uint32).reshape(-1)
    w = np.asarray(weight).reshape(-1)
    if len(w) != n or (len(w) and (w.min() < 0 or w.max() > 0xFFFF)):
        raise ValueError("one weight of 1..65535 per end point expected")
    w = np.ascontiguousarray(w, dtype=np.uint16)
    spec = _capi.pg_reach_cost_spec(matrix_ptr, int(n), int(n_svc), sel.ctypes.data if sel is not None else None,
                                    s.ctypes.data if len(s) else None, len(s), w.ctypes.data if len(w) else None, int(max_cost))
    return spec, (sel, s, w)


def cost_result(res):
    return {name: getattr(res, name) for name, _ in res._fields_}


def reach_cost(engine, matrix, n, n_svc, src, weight, max_cost=0, svc_select=None, cost=True, pred=False, len=False, via=False,
               stream=None):
    """The cheapest walks from the end points ``src`` when taking end point v costs ``weight[v]`` (1..65535;
    the source is held and costs nothing), over the ALLOW graph of a square reach_matrix result, on the GPU
    (pg_reach_cost). ``matrix`` is an int32 device tensor [n_svc, n, row_words(n)] taken with one end-point
    list on both sides; ``src`` are ids (duplicates allowed); ``svc_select`` (one flag per slice, None = all)
    says which slices contribute edges; with ``max_cost`` != 0 only cells of at most that cost are reached.
    -> (cost, pred, len, via, result): with ``cost`` the costs as an int32 tensor [n_src, n] (view it as
    uint32: NO_COST where not reached), with ``pred`` the least predecessors and with ``len`` the edges of
    the cheapest paths as int16 tensors [n_src, n] (view them as uint16: NO_PRED and 0 where not reached),
    with ``via`` the cheapest paths that cross each end point as an int32 tensor [n], and {n_reached, n_via,
    max_cost, longest}. Whatever was not asked for is None. The call never touches the hit counters."""
    rw = reach_row_words(n)
    if matrix.dtype != torch.int32 or not matrix.is_contiguous() or matrix.numel() != n_svc * n * rw:
        raise ValueError("a contiguous int32 tensor [n_svc, n, row_words(n)] expected")
    spec, keep = cost_spec(matrix.data_ptr() if n else None, n, n_svc, src, weight, max_cost, svc_select)
    new = lambda dtype: torch.empty((spec.n_src, n), dtype=dtype, device="cuda")
    c, p, ln = new(torch.int32) if cost else None, new(torch.int16) if pred else None, new(torch.int16) if len else None
    v = torch.empty(n, dtype=torch.int32, device="cuda") if via else None
    res = _capi.pg_reach_cost_result()
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    engine._ck(lib.pg_reach_cost(engine.h, C.byref(spec), ptr(c), ptr(p), ptr(ln), ptr(v), C.byref(res), _stream_ptr(stream)))
    del keep
    return c, p, ln, v, cost_result(res)


# ---- observed reachability (include/policygpu.h pg_reach_observed) ---------------------------
def observed_spec(src_ips, dst_ips, services, flags=0):
    """pg_reach_observed_spec over host arrays (reach_spec's, and the PG_OBSERVED_* flags) -> (spec,
    the arrays it points into: keep them alive for the call)"""
    src = np.ascontiguousarray(src_ips, dtype=np.uint32)
    dst = np.ascontiguousarray(dst_ips, dtype=np.uint32)
    svc = (_capi.pg_service * max(1, len(services)))()
    for i, (proto, sport, dport) in enumerate(services):
        svc[i].protocol, svc[i].src_port, svc[i].dst_port = int(proto), int(sport), int(dport)
    spec = _capi.pg_reach_observed_spec(src.ctypes.data if len(src) else None, len(src), dst.ctypes.data if len(dst) else None,
                                        len(dst), svc, len(services), int(flags))
    return spec, (src, dst, svc)


def observed_result(res):
    return {"n_matched": res.n_matched, "n_no_src": res.n_no_src, "n_no_dst": res.n_no_dst, "n_no_svc": res.n_no_svc,
            "n_cells": res.n_cells}


def reach_observed(engine, src_ips, dst_ips, services, batch, n=None, match_src_port=False, into=None, flow=False,
                   svc_flows=False, stream=None):
    """A flow log folded into reach_matrix's layout, on the GPU (pg_reach_observed): cell (v, i, j) is ALLOW
    where some flow of the TupleBatch ``batch`` (its first ``n``) went from src_ips[i] to dst_ips[j] on
    services[v] (protocol, src port, dst port; the src port counts only with ``match_src_port``), DENY_SYN
    elsewhere. -> (packed, flow, svc_flows, result): the int32 tensor [n_svc, n_src, row_words] -- ``into``,
    an earlier result of the same lists, is ORed into and returned -- with ``flow`` the PG_OBS_* status of
    every flow as a uint8 tensor [n], with ``svc_flows`` the matched flows of every service as an int64
    tensor [n_svc], and {n_matched, n_no_src, n_no_dst, n_no_svc, n_cells}. Whatever was not asked for is
    None. The result compares with reach_matrix's by reach_diff. The call never touches the hit counters."""
    flags = (_capi.OBSERVED_MATCH_SRC_PORT if match_src_port else 0) | (_capi.OBSERVED_ACCUMULATE if into is not None else 0)
    spec, keep = observed_spec(src_ips, dst_ips, services, flags)
    n = batch.n if n is None else int(n)
    shape = (len(services), spec.n_src, reach_row_words(spec.n_dst))
    if into is not None:
        if into.dtype != torch.int32 or not into.is_contiguous() or tuple(into.shape) != shape:
            raise ValueError("a contiguous int32 tensor [n_svc, n_src, row_words(n_dst)] expected")
        packed = into
    else:
        packed = torch.empty(shape, dtype=torch.int32, device="cuda")
    out_flow = torch.empty(n, dtype=torch.uint8, device="cuda") if flow else None
    counts = torch.empty(len(services), dtype=torch.int64, device="cuda") if svc_flows else None
    res = _capi.pg_reach_observed_result()
    soa = batch.soa()
    if not match_src_port:
        soa.src_port = None
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    # (an empty matrix has no address to hand over, but the call wants one: nothing is written through it)
    engine._ck(lib.pg_reach_observed(engine.h, C.byref(spec), C.byref(soa), n, ptr(packed) or 16, ptr(out_flow), ptr(counts),
                                     C.byref(res), _stream_ptr(stream)))
    del keep
    return packed, out_flow, counts, observed_result(res)


# ---- rule coverage (include/policygpu.h pg_reach_rules) ---------------------------------------
def rules_spec(src_ips, dst_ips, services, weights, n_slots):
    """pg_reach_rules_spec over host arrays (reach_spec's, and the weights as u32 or None) -> (spec,
    the arrays it points into: keep them alive for the call)"""
    rs, keep = reach_spec(src_ips, dst_ips, services)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.uint32)
    if w is not None and len(w) != len(services):
        raise ValueError("one weight per service expected")
    spec = _capi.pg_reach_rules_spec(rs.src_ip, rs.n_src, rs.dst_ip, rs.n_dst, rs.services, rs.n_svc,
                                     w.ctypes.data if w is not None and len(w) else None, int(n_slots))
    return spec, (keep, w)


def rules_result(res):
    return {"n_slots": res.n_slots, "layout_gen": res.layout_gen, "n_cells": res.n_cells, "n_evals": res.n_evals,
            "n_rule_slots": res.n_rule_slots, "n_dead_rules": res.n_dead_rules}


def reach_rules(engine, src_ips, dst_ips, services, weights=None, evals=True, cells=True, stream=None):
    """Per-rule coverage of the product src x dst x services on the GPU (pg_reach_rules), without the
    product: -> (evals, cells, result). ``evals`` an int64 tensor [n_slots], the weighted evalACL
    evaluations each counter slot decided (what pg_classify CONN would add to zeroed counters over the
    product's tuples); ``cells`` an int64 tensor [n_slots, 4], the weighted cells by deciding slot and
    ConnAction (the histogram of reach_matrix's words); whichever was not asked for is None. ``weights``
    (0 .. 65536 per service, None = 1) repeat a slice. result: {n_slots, layout_gen, n_cells, n_evals,
    n_rule_slots, n_dead_rules}. The call never touches the hit counters."""
    if not (evals or cells):
        raise ValueError("at least one of evals and cells")
    n_slots = engine.num_counter_slots()
    spec, keep = rules_spec(src_ips, dst_ips, services, weights, n_slots)
    ev = torch.empty(n_slots, dtype=torch.int64, device="cuda") if evals else None
    ce = torch.empty((n_slots, 4), dtype=torch.int64, device="cuda") if cells else None
    res = _capi.pg_reach_rules_result()
    engine._ck(lib.pg_reach_rules(engine.h, C.byref(spec), ev.data_ptr() if evals else None,
                                  ce.data_ptr() if cells else None, C.byref(res), _stream_ptr(stream)))
    del keep
    return ev, ce, rules_result(res)


def unpack(out_u32):
    w = out_u32.astype(np.uint32)
    return (w >> 30).astype(np.int64), (w & 0x3FFFFFFF).astype(np.int64)
