"""Python face of the engine, mirroring the reference's interfaces for this path.

Names follow the reference so parity tests read like its own tests:

* ``ContivRule``, ``ActionType``, ``ProtocolType``     renderer/api.go:65-176
* ``Renderer.NewTxn`` / ``Txn.Render`` / ``Txn.Commit``  renderer/api.go:33-61 (PolicyRendererAPI)
* ``Engine.RegisterPod`` / ``Connection*`` / ``GetNumOfACLs`` / ``GetInboundACL`` ...
                                                       mock/aclengine/aclengine_mock.go
* ``Engine.SetPodIfName`` / ``SetVxlanBVIIfName`` / ...  mock/ipv4net/ipv4net_mock.go:40-66

Everything below delegates to the C ABI (``_capi``); evalACL / testConnection run on the GPU.
"""
import ctypes as C
import ipaddress
import json

from . import _capi
from ._capi import lib

# renderer.ActionType / ProtocolType (api.go:140-176)
ActionDeny, ActionPermit = 0, 1
TCP, UDP, OTHER, ANY = 0, 1, 2, 3
# aclengine ConnectionAction / ACLAction (aclengine_mock.go:39-71)
ConnActionDenySyn, ConnActionDenySynAck, ConnActionAllow, ConnActionFailure = 0, 1, 2, 3
ACLActionDeny, ACLActionPermit, ACLActionReflect, ACLActionFailure = 0, 1, 2, 3
# cache.Orientation
IngressOrientation, EgressOrientation = 0, 1


class PolicyError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (code %d)" % (msg, code))
        self.code = code


def _b(s):
    return s.encode() if isinstance(s, str) else s


class IPNet:
    """net.IPNet: ``IPNet()`` is the empty network (match all); ``IPNet("10.0.0.0/8")`` parses a
    CIDR (keeping the address as written, like a Go IPNet built by hand would)."""

    __slots__ = ("family", "prefix_len", "addr")

    def __init__(self, cidr=None):
        if not cidr:
            self.family, self.prefix_len, self.addr = 0, 0, b""
            return
        ip, _, plen = cidr.partition("/")
        a = ipaddress.ip_address(ip)
        self.family = a.version
        self.addr = a.packed
        self.prefix_len = int(plen) if plen else (32 if a.version == 4 else 128)

    @classmethod
    def host(cls, ip):
        """utils.GetOneHostSubnet (utils.go:271-291)."""
        n = cls(ip)
        n.prefix_len = 32 if n.family == 4 else 128
        return n

    def c(self):
        v = _capi.pg_ipnet()
        v.family = self.family
        v.prefix_len = self.prefix_len
        for i, x in enumerate(self.addr):
            v.addr[i] = x
        return v

    def __repr__(self):
        if not self.family:
            return "ANY"
        return "%s/%d" % (ipaddress.ip_address(self.addr), self.prefix_len)


class ContivRule:
    """renderer.ContivRule (api.go:65-77)."""

    __slots__ = ("Action", "SrcNetwork", "DestNetwork", "Protocol", "SrcPort", "DestPort")

    def __init__(self, Action=ActionPermit, SrcNetwork=None, DestNetwork=None, Protocol=ANY, SrcPort=0, DestPort=0):
        self.Action = Action
        self.SrcNetwork = SrcNetwork if isinstance(SrcNetwork, IPNet) else IPNet(SrcNetwork)
        self.DestNetwork = DestNetwork if isinstance(DestNetwork, IPNet) else IPNet(DestNetwork)
        self.Protocol = Protocol
        self.SrcPort = SrcPort
        self.DestPort = DestPort

    def c(self):
        r = _capi.pg_contiv_rule()
        r.action, r.protocol, r.src_port, r.dst_port = self.Action, self.Protocol, self.SrcPort, self.DestPort
        r.src = self.SrcNetwork.c()
        r.dst = self.DestNetwork.c()
        return r

    def __repr__(self):
        return "Rule <%s %s[%d:%d] -> %s[%d:%d]>" % (
            "PERMIT" if self.Action else "DENY", self.SrcNetwork, self.Protocol, self.SrcPort, self.DestNetwork,
            self.Protocol, self.DestPort)


def _rules_array(rules):
    arr = (_capi.pg_contiv_rule * max(1, len(rules)))()
    for i, r in enumerate(rules):
        arr[i] = r.c()
    return arr, len(rules)


def _pod(pod):
    """podmodel.ID as "namespace/name" or (namespace, name)."""
    if isinstance(pod, str):
        ns, _, name = pod.partition("/")
        return ns, name
    return pod


class Engine:
    """The device ACL engine (one GPU): MockACLEngine's API + ipv4net/contivconf setters."""

    def __init__(self, device=0):
        self.h = lib.pg_create(device)
        if not self.h:
            raise PolicyError(_capi.PG_ENOMEM, "pg_create failed")
        self._keep = []
        self.registered_pods = {}  # "ns/name" -> (IP, anotherNode) as given to RegisterPod

    def close(self):
        if self.h:
            lib.pg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc < 0:
            raise PolicyError(rc, lib.pg_last_error(self.h).decode())
        return rc

    # tuning knobs of this context (pg_ctx_set_tuning; include/policygpu.h lists the keys)
    def set_tuning(self, key, value):
        self._ck(lib.pg_ctx_set_tuning(self.h, _b(key), int(value)))

    def get_tuning(self, key):
        v = C.c_int()
        self._ck(lib.pg_ctx_get_tuning(self.h, _b(key), C.byref(v)))
        return v.value

    def tuning(self, **kw):
        """context manager: the given knobs set for the block, restored afterwards"""
        import contextlib

        @contextlib.contextmanager
        def cm():
            old = {k: self.get_tuning(k) for k in kw}
            try:
                for k, v in kw.items():
                    self.set_tuning(k, v)
                yield self
            finally:
                for k, v in old.items():
                    self.set_tuning(k, v)
        return cm()

    @property
    def device(self):
        return self._ck(lib.pg_ctx_device(self.h))

    # ipv4net / contivconf setters
    def SetPodIfName(self, pod, if_name):
        ns, name = _pod(pod)
        self._ck(lib.pg_set_pod_if_name(self.h, _b(ns), _b(name), _b(if_name)))

    def SetHostInterconnectIfName(self, n):
        self._ck(lib.pg_set_host_interconnect_if_name(self.h, _b(n)))

    def SetMainInterfaceName(self, n):
        self._ck(lib.pg_set_main_interface_name(self.h, _b(n)))

    def SetOtherVPPInterfaces(self, names):
        arr = (C.c_char_p * max(1, len(names)))(*[_b(x) for x in names])
        self._ck(lib.pg_set_other_vpp_interfaces(self.h, arr, len(names)))

    def SetVxlanBVIIfName(self, n):
        self._ck(lib.pg_set_vxlan_bvi_if_name(self.h, _b(n)))

    def RegisterPod(self, pod, ip, another_node):
        ns, name = _pod(pod)
        self._ck(lib.pg_register_pod(self.h, _b(ns), _b(name), _b(ip), int(another_node)))
        self.registered_pods["%s/%s" % (ns, name)] = (ip, bool(another_node))

    # ACL install / introspection
    def ApplyTxn(self, resync, ops):
        """ops: list of (key, acl dict or None); acl dicts as returned by GetACLByName."""
        keep = []
        arr = (_capi.pg_acl_op * max(1, len(ops)))()
        for i, (key, acl) in enumerate(ops):
            arr[i].key = _b(key)
            if acl is not None:
                a = _acl_struct(acl, keep)
                keep.append(a)
                arr[i].value = C.pointer(a)
        return self._ck(lib.pg_apply_txn(self.h, int(resync), arr, len(ops)))

    def GetNumOfACLs(self):
        return self._ck(lib.pg_num_acls(self.h))

    def GetNumOfACLChanges(self):
        return self._ck(lib.pg_num_acl_changes(self.h))

    def NumCommittedTxns(self):
        return self._ck(lib.pg_num_committed_txns(self.h))

    def GetACLByName(self, name):
        n = lib.pg_acl_json(self.h, _b(name), None, 0)
        if n == _capi.PG_ENOENT:
            return None
        self._ck(n)
        buf = C.create_string_buffer(n)
        self._ck(lib.pg_acl_json(self.h, _b(name), buf, n))
        return json.loads(buf.value.decode())

    def ACLNames(self):
        n = self._ck(lib.pg_acl_names_json(self.h, None, 0))
        buf = C.create_string_buffer(n)
        self._ck(lib.pg_acl_names_json(self.h, buf, n))
        return json.loads(buf.value.decode())

    def _if_acls(self, if_name):
        a, b = C.create_string_buffer(512), C.create_string_buffer(512)
        self._ck(lib.pg_interface_acls(self.h, _b(if_name), a, 512, b, 512))
        return a.value.decode(), b.value.decode()

    def GetInboundACL(self, if_name):
        n = self._if_acls(if_name)[0]
        return self.GetACLByName(n) if n else None

    def GetOutboundACL(self, if_name):
        n = self._if_acls(if_name)[1]
        return self.GetACLByName(n) if n else None

    # device tables
    def sync(self):
        self._ck(lib.pg_sync_tables(self.h))

    def table_id(self, acl_name):
        return self._ck(lib.pg_table_id(self.h, _b(acl_name)))

    def num_tables(self):
        return self._ck(lib.pg_num_tables(self.h))

    def num_counter_slots(self):
        return self._ck(lib.pg_num_counter_slots(self.h))

    def slot_info(self, slot):
        t, r = C.c_int32(), C.c_int32()
        self._ck(lib.pg_slot_info(self.h, slot, C.byref(t), C.byref(r)))
        return t.value, r.value

    def table_info(self, tid):
        b, n, d = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._ck(lib.pg_table_info(self.h, tid, C.byref(b), C.byref(n), C.byref(d)))
        return b.value, n.value, d.value

    def table_stats(self, tid):
        v = [C.c_uint32() for _ in range(4)]
        self._ck(lib.pg_table_stats(self.h, tid, *[C.byref(x) for x in v]))
        f, nbytes, nsc, nkc = (x.value for x in v)
        mode = "linear" if f & 8 else ("fd" if f & 32 else ("pair" if f & 16 else ("candi" if f & 128 else (
            "cand" if f & 4 else ("cross+lists" if f & 2 else "cross")))))
        return {"structure": mode, "blob_bytes": nbytes, "src_classes": nsc, "key_classes": nkc,
                "dst_free": bool(f & 64)}

    def debug_walk(self, acl_name, src, dst, dport, proto):
        """TESTS ONLY: host walk of the ACL's compiled blob (see pg_debug_walk_blob)."""
        import numpy as np
        n = len(src)
        a = [np.ascontiguousarray(x, dt) for x, dt in ((src, np.uint32), (dst, np.uint32), (dport, np.uint16),
                                                       (proto, np.uint8))]
        out = np.empty(n, np.uint32)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        self._ck(lib.pg_debug_walk_blob(self.h, _b(acl_name), p(a[0]), p(a[1]), p(a[2]), p(a[3]), n, p(out)))
        return out

    def debug_classify_host(self, mode, table_id, src, dst, sport, dport, proto, counters=False, node=True,
                            pred=True, common=True):
        """TESTS ONLY: pg_classify's per-tuple code run on the host (pg_debug_classify_host).
        ``common``: the node image's common-row section (when it was built).
        -> verdict words (u32), and the u64 hit counters when ``counters``."""
        import numpy as np
        n = len(src)
        a = [np.ascontiguousarray(x, dt) for x, dt in ((src, np.uint32), (dst, np.uint32), (sport, np.uint16),
                                                       (dport, np.uint16), (proto, np.uint8))]
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        t = _capi.pg_tuple_soa(p(a[0]), p(a[1]), p(a[2]), p(a[3]), p(a[4]))
        out = np.empty(n, np.uint32)
        cnt = np.zeros(self.num_counter_slots(), np.uint64) if counters else None
        self._ck(lib.pg_debug_classify_host(self.h, mode, table_id, C.byref(t), n, p(out),
                                            p(cnt) if counters else None,
                                            int(node) | (2 if pred else 0) | (4 if common else 0)))
        return (out, cnt) if counters else out

    def debug_endpoint_probe(self, ips):
        """TESTS ONLY: where the end-point hash table finds each address (pg_debug_endpoint_probe).
        -> (probe steps u32 [n], start slot u32 [n], the table's capacity)"""
        import numpy as np
        ips = np.ascontiguousarray(ips, dtype=np.uint32)
        steps, slot, cap = np.zeros(len(ips), np.uint32), np.zeros(len(ips), np.uint32), C.c_uint32()
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        self._ck(lib.pg_debug_endpoint_probe(self.h, p(ips), len(ips), p(steps), p(slot), C.byref(cap)))
        return steps, slot, cap.value

    def debug_reach_matrix_host(self, src_ips, dst_ips, services, words=True, node=True):
        """TESTS ONLY: pg_reach_matrix's code run on the host (pg_debug_reach_matrix_host).
        services: (protocol, src port, dst port). -> packed u32 [n_svc, n_src, row_words], and the
        full verdict words u32 [n_svc, n_src, n_dst] when ``words``."""
        import numpy as np
        from . import device as D
        spec, (src, dst, _svc) = D.reach_spec(src_ips, dst_ips, services)
        rw = lib.pg_reach_row_words(len(dst))
        packed = np.full((len(services), len(src), rw), 0xFFFFFFFF, np.uint32)
        full = np.full((len(services), len(src), len(dst)), 0xFFFFFFFF, np.uint32) if words else None
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        self._ck(lib.pg_debug_reach_matrix_host(self.h, C.byref(spec), p(packed), p(full) if words else None,
                                                int(node)))
        return (packed, full) if words else packed

    def _pod_ips(self, pods):
        """registered IPv4 addresses of "ns/name" pods as u32"""
        out = []
        for pod in pods:
            key = "%s/%s" % _pod(pod)
            if key not in self.registered_pods:
                raise PolicyError(_capi.PG_ENOENT, "pod %s is not registered" % key)
            out.append(int(ipaddress.IPv4Address(self.registered_pods[key][0])))
        return out

    def reachability(self, src_pods, dst_pods, services, host=False):
        """Which pods reach which, on which services: the ConnAction of every (service, src pod,
        dst pod), a uint8 array [n_svc, n_src, n_dst], by one pg_reach_matrix call. Pods are
        "ns/name" (or (ns, name)), resolved through the addresses given to RegisterPod; services
        are (protocol, src port, dst port). ``host``: TESTS ONLY, the host twin instead of the GPU."""
        from . import device as D
        src, dst = self._pod_ips(src_pods), self._pod_ips(dst_pods)
        if host:
            packed = self.debug_reach_matrix_host(src, dst, services, words=False)
        else:
            import torch
            packed = D.reach_matrix(self, src, dst, services)
            torch.cuda.synchronize()
        return D.unpack_reach(packed, len(services), len(src), len(dst))

    def port_intervals(self, protocol):
        """lower bounds lo[K] (uint32, lo[0] = 0, ascending) of the elementary dst-port intervals of
        TCP (0) or UDP (1) over the installed ACLs (pg_port_intervals): inside one interval every
        pair has one verdict"""
        from . import device as D
        return D.port_intervals(self, protocol)

    def debug_reach_ports_host(self, src_ips, dst_ips, protocol, src_port=40000, node=True, n_intervals=None):
        """TESTS ONLY: pg_reach_ports's code run on the host (pg_debug_reach_ports_host).
        -> (lo u32[K], codes u32 [n_src, n_dst, row_words(K)], open u32 [n_src, n_dst], words u32
        [n_src, n_dst, K]); the outputs are pre-filled with 0xFFFFFFFF."""
        import numpy as np
        from . import device as D
        lo = self.port_intervals(protocol)
        k = len(lo) if n_intervals is None else n_intervals
        spec, keep = D.ports_spec(src_ips, dst_ips, protocol, src_port, k)
        codes = np.full((spec.n_src, spec.n_dst, lib.pg_reach_row_words(k)), 0xFFFFFFFF, np.uint32)
        n_open = np.full((spec.n_src, spec.n_dst), 0xFFFFFFFF, np.uint32)
        full = np.full((spec.n_src, spec.n_dst, k), 0xFFFFFFFF, np.uint32)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        self._ck(lib.pg_debug_reach_ports_host(self.h, C.byref(spec), p(codes), p(n_open), p(full), int(node)))
        del keep
        return lo, codes, n_open, full

    def open_ports(self, src_pods, dst_pods, protocol, src_port=40000, host=False):
        """Between these pods, which dst ports are open? One pg_reach_ports call over all 65,536 dst
        ports of TCP (0) or UDP (1). -> (ranges, open): ranges[i][j] the maximal (lo, hi) port
        ranges, ascending, on which src pod i reaches dst pod j (ConnAction ALLOW; adjacent ALLOW
        intervals merged), open a uint32 array [n_src, n_dst] of how many ports that is. Pods as in
        reachability. ``host``: TESTS ONLY, the host twin instead of the GPU."""
        import numpy as np
        from . import device as D
        src, dst = self._pod_ips(src_pods), self._pod_ips(dst_pods)
        if host:
            lo, codes, n_open, _ = self.debug_reach_ports_host(src, dst, protocol, src_port)
        else:
            import torch
            lo, codes, n_open = D.reach_ports(self, src, dst, protocol, src_port, open_count=True)
            torch.cuda.synchronize()
            n_open = n_open.cpu().numpy().view(np.uint32)
        allow = D.unpack_ports(codes, len(src), len(dst), len(lo)) == 2   # PG_CONN_ALLOW
        # a range starts where ALLOW begins and ends where it stops: the edges of the 0-padded row
        edge = np.diff(np.pad(allow.astype(np.int8), ((0, 0), (0, 0), (1, 1))), axis=2)
        hi = np.append(lo[1:], 65536).astype(np.int64) - 1
        ranges = [[list(zip(lo[edge[i, j, :-1] == 1].tolist(), hi[edge[i, j, 1:] == -1].tolist()))
                   for j in range(len(dst))] for i in range(len(src))]
        return ranges, n_open

    def debug_reach_diff_host(self, before, after, n_cols, transitions=_capi.DIFF_ALL, cap=None, row_changes=True):
        """TESTS ONLY: pg_reach_diff's per-word code run on the host (pg_debug_reach_diff_host) over
        numpy arrays of packed words [..., row_words(n_cols)]. ``cap`` None: as many entries as there
        are cells. -> (n_changes, changes u32 [cap, 2], trans u64 [4, 4], row_changes u32 [n_rows] or
        None); changes and row_changes are pre-filled with 0xFFFFFFFF."""
        import numpy as np
        b = np.ascontiguousarray(before, dtype=np.uint32)
        a = np.ascontiguousarray(after, dtype=np.uint32)
        rw = lib.pg_reach_row_words(n_cols)
        n_rows = b.size // rw
        cap = n_rows * int(n_cols) if cap is None else cap
        changes = np.full((cap, 2), 0xFFFFFFFF, np.uint32)
        rows = np.full(n_rows, 0xFFFFFFFF, np.uint32) if row_changes else None
        trans = np.full(16, 0xFFFFFFFFFFFFFFFF, np.uint64)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        spec = _capi.pg_reach_diff_spec(b.ctypes.data, a.ctypes.data, n_rows, int(n_cols), int(transitions), cap)
        n = C.c_uint64()
        self._ck(lib.pg_debug_reach_diff_host(self.h, C.byref(spec), p(changes) if cap else None,
                                              p(rows) if row_changes else None, C.byref(n), p(trans)))
        return n.value, changes, trans.reshape(4, 4), rows

    def debug_reach_diff_plan(self, n_words):
        """TESTS ONLY: how pg_reach_diff cuts n_words words under this context's knobs
        (pg_debug_reach_diff_plan) -> {tile_words, grid, chunk_words}"""
        t, g, c = C.c_uint32(), C.c_uint32(), C.c_uint64()
        self._ck(lib.pg_debug_reach_diff_plan(self.h, int(n_words), C.byref(t), C.byref(g), C.byref(c)))
        return {"tile_words": t.value, "grid": g.value, "chunk_words": c.value}

    def reachability_diff(self, baseline, src_pods, dst_pods, services, transitions=_capi.DIFF_ALL, host=False):
        """What a policy change opened or closed: the (service, src pod, dst pod) whose ConnAction
        under this engine differs from that under ``baseline`` (another Engine on the same device),
        by two pg_reach_matrix calls and one pg_reach_diff. -> ([(service index, src pod, dst pod,
        ConnAction before, after), ...] in (service, src, dst) order with the pods as given,
        trans): ``transitions`` selects what is listed (DIFF_OPENED, DIFF_CLOSED, ...), trans is the
        uint64 array [before, after] over all pairs. ``host``: TESTS ONLY, the host twins."""
        from . import device as D
        src, dst = self._pod_ips(src_pods), self._pod_ips(dst_pods)
        if host:
            b = baseline.debug_reach_matrix_host(src, dst, services, words=False)
            a = self.debug_reach_matrix_host(src, dst, services, words=False)
            n, changes, trans, _ = self.debug_reach_diff_host(b, a, len(dst), transitions, row_changes=False)
            changes = changes[:n]
        else:
            b = D.reach_matrix(baseline, src, dst, services)
            a = D.reach_matrix(self, src, dst, services)
            n, changes, trans, _ = D.reach_diff(self, b, a, len(dst), transitions)
        row, col, cb, ca = D.unpack_changes(changes)
        ns = max(1, len(src))
        out = [(int(r) // ns, src_pods[int(r) % ns], dst_pods[int(j)], int(x), int(y))
               for r, j, x, y in zip(row, col, cb, ca)]
        return out, trans

    def debug_reach_closure_host(self, matrix, n, svc_select=None, max_hops=0, hops=True, counts=True):
        """TESTS ONLY: pg_reach_closure's per-word code run on the host (pg_debug_reach_closure_host)
        over a numpy array of packed words [n_svc, n, row_words(n)]. -> (packed u32 [n, row_words(n)],
        hops u16 [n, n] or None, counts u32 [n] or None, {levels, n_edges, n_reachable}); the outputs
        are pre-filled with 0xFF.."""
        import numpy as np
        from . import device as D
        m = np.ascontiguousarray(matrix, dtype=np.uint32)
        rw = lib.pg_reach_row_words(n)
        n_svc = m.size // max(1, n * rw)
        packed = np.full((n, rw), 0xFFFFFFFF, np.uint32)
        hop = np.full((n, n), 0xFFFF, np.uint16) if hops else None
        cnt = np.full(n, 0xFFFFFFFF, np.uint32) if counts else None
        res = _capi.pg_reach_closure_result()
        if n == 0:
            return packed, hop, cnt, D.closure_result(res)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        spec, keep = D.closure_spec(m.ctypes.data, n, n_svc, svc_select, max_hops)
        self._ck(lib.pg_debug_reach_closure_host(self.h, C.byref(spec), p(packed), p(hop) if hops else None,
                                                 p(cnt) if counts else None, C.byref(res)))
        del keep
        return packed, hop, cnt, D.closure_result(res)

    def debug_reach_closure_plan(self, n):
        """TESTS ONLY: how one level of pg_reach_closure over n end points is cut
        (pg_debug_reach_closure_plan) -> {tile_rows, tile_cols, grid}"""
        r, c, g = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._ck(lib.pg_debug_reach_closure_plan(self.h, int(n), C.byref(r), C.byref(c), C.byref(g)))
        return {"tile_rows": r.value, "tile_cols": c.value, "grid": g.value}

    def _closure(self, ips, services, max_hops, host, hops):
        """one pg_reach_matrix over ips x ips and one closure of all its slices -> (packed, hops,
        result), device tensors or with ``host`` numpy arrays"""
        from . import device as D
        n = len(ips)
        if host:
            m = self.debug_reach_matrix_host(ips, ips, services, words=False)
            packed, hop, _, res = self.debug_reach_closure_host(m, n, None, max_hops, hops=hops, counts=False)
        else:
            m = D.reach_matrix(self, ips, ips, services)
            packed, hop, _, res = D.reach_closure(self, m, n, None, max_hops, hops=hops)
        return packed, hop, res

    def reachability_closure(self, pods, services, max_hops=0, host=False):
        """Lateral movement: which pods a pod gets to by hopping through the pods it reaches on any of
        ``services``, and in how many hops, by one pg_reach_matrix over pods x pods and one
        pg_reach_closure. -> (reach bool [n, n], hops uint16 [n, n] (0 = not reachable), levels) with
        the pods as given; ``max_hops`` 0 = no bound. Pods and services as in reachability. ``host``:
        TESTS ONLY, the host twins instead of the GPU."""
        import numpy as np
        from . import device as D
        ips = self._pod_ips(pods)
        n = len(ips)
        if n == 0 or not services:
            return np.zeros((n, n), bool), np.zeros((n, n), np.uint16), 0
        packed, hop, res = self._closure(ips, services, max_hops, host, True)
        if not host:
            hop = hop.cpu().numpy().view(np.uint16)
        return D.unpack_closure(packed, n), hop, res["levels"]

    def reachability_closure_diff(self, baseline, pods, services, transitions=_capi.DIFF_OPENED, max_hops=0, host=False,
                                  paths=False):
        """What a policy change opened (or closed) transitively: the (src pod, dst pod) whose cell of
        the closure under this engine differs from that under ``baseline`` (another Engine on the same
        device), by two pg_reach_matrix calls, two pg_reach_closure calls and one pg_reach_diff over
        the closures. -> [(src pod, dst pod, before, after), ...] in (src, dst) order with the pods as
        given; before / after are ConnActions, ALLOW = reachable and DENY_SYN = not. With ``paths`` every
        entry has a fifth member: for a cell that is reachable after, its path under this engine as a
        list of pods (one pg_reach_paths call, the diff's changes being the queries), else None.
        ``host``: TESTS ONLY, the host twins."""
        from . import device as D
        ips = self._pod_ips(pods)
        n = len(ips)
        if n == 0 or not services:
            return []
        b, _, _ = baseline._closure(ips, services, max_hops, host, False)
        a, hop, _ = self._closure(ips, services, max_hops, host, paths)
        if host:
            k, changes, _, _ = self.debug_reach_diff_host(b, a, n, transitions, row_changes=False)
            changes = changes[:k]
        else:
            _, changes, _, _ = D.reach_diff(self, b, a, n, transitions)
        row, col, cb, ca = D.unpack_changes(changes)
        out = [(pods[int(r)], pods[int(j)], int(x), int(y)) for r, j, x, y in zip(row, col, cb, ca)]
        if not paths:
            return out
        found = self._paths(hop, n, row, col, host)
        return [t + (None if p is None else [pods[k] for k in p],) for t, p in zip(out, found)]

    def debug_reach_paths_host(self, hops, n, src, dst, max_len=None, nodes=True, via=True):
        """TESTS ONLY: pg_reach_paths's per-word code, partition and plan run on the host
        (pg_debug_reach_paths_host) over a numpy array of hop counts [n, n]. -> (lengths u16 [n_queries],
        nodes u16 [n_queries, max_len + 1] or None, via u32 [n] or None, {n_found, ...}); the outputs are
        pre-filled with 0xFF.. (the nodes with 0xEEEE)."""
        import numpy as np
        from . import device as D
        h = np.ascontiguousarray(hops, dtype=np.uint16)
        max_len = max(1, n) if max_len is None else int(max_len)
        spec, keep = D.paths_spec(h.ctypes.data, n, src, dst, max_len)
        nq = int(spec.n_queries)
        lens = np.full(nq, 0xFFFF, np.uint16)
        rows = np.full((nq, max_len + 1), 0xEEEE, np.uint16) if nodes else None
        cnt = np.full(n, 0xFFFFFFFF, np.uint32) if via else None
        res = _capi.pg_reach_paths_result()
        if n == 0:
            return lens, rows, cnt, D.paths_result(res)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        self._ck(lib.pg_debug_reach_paths_host(self.h, C.byref(spec), p(lens) if nq else p(h), p(rows) if nodes and nq else None,
                                               p(cnt) if via else None, C.byref(res)))
        del keep
        return lens, rows, cnt, D.paths_result(res)

    def debug_reach_paths_plan(self, n):
        """TESTS ONLY: how pg_reach_paths over n end points is cut (pg_debug_reach_paths_plan) ->
        {chunk_queries, lds_bytes}"""
        c, b = C.c_uint32(), C.c_uint32()
        self._ck(lib.pg_debug_reach_paths_plan(self.h, int(n), C.byref(c), C.byref(b)))
        return {"chunk_queries": c.value, "lds_bytes": b.value}

    def _paths(self, hop, n, src, dst, host, via=False):
        """one pg_reach_paths over a _closure's hops (a device tensor, or with ``host`` a numpy array) ->
        one list of node indices per query, None where there is no path; with ``via`` the uint32 counts
        [n] instead"""
        import numpy as np
        from . import device as D
        if host:
            lens, rows, cnt, _ = self.debug_reach_paths_host(hop, n, src, dst, nodes=not via, via=via)
        else:
            lens, rows, cnt, _ = D.reach_paths(self, hop, n, src, dst, nodes=not via, via=via)
            if via:
                cnt = cnt.cpu().numpy().view(np.uint32)
        return cnt if via else D.unpack_paths(lens, rows)

    def reachability_paths(self, pods, services, pairs, max_hops=0, host=False):
        """Through which pods: for every (src pod, dst pod) of ``pairs``, both among ``pods``, one
        shortest path over the graph of reachability_closure, by one pg_reach_matrix over pods x pods,
        one pg_reach_closure and one pg_reach_paths. -> one list of pods per pair, from the src to the
        dst (a pod paired with itself: its shortest cycle), None where the dst is not reachable (within
        ``max_hops`` edges when that is set). Of several shortest paths it is the one the
        least-predecessor rule of include/policygpu.h defines, in the order of ``pods``. Pods and
        services as in reachability. ``host``: TESTS ONLY, the host twins."""
        ips = self._pod_ips(pods)
        n = len(ips)
        pairs = list(pairs)
        if n == 0 or not services or not pairs:
            return [None] * len(pairs)
        index = {pod: k for k, pod in reversed(list(enumerate(pods)))}
        src, dst = [index[a] for a, _ in pairs], [index[b] for _, b in pairs]
        _, hop, _ = self._closure(ips, services, max_hops, host, True)
        found = self._paths(hop, n, src, dst, host)
        return [None if p is None else [pods[k] for k in p] for p in found]

    def reachability_chokepoints(self, pods, services, sources=None, targets=None, max_hops=0, host=False):
        """Which pod to lock down: over the shortest paths (as reachability_paths picks them) from every
        pod of ``sources`` to every pod of ``targets`` (both among ``pods``; None = all of them), how many
        pass through each pod, by one pg_reach_matrix, one pg_reach_closure and one pg_reach_paths that
        returns the counts alone. -> [(pod, count), ...] of the pods with a count, by descending count and
        then in the order of ``pods``. ``host``: TESTS ONLY, the host twins."""
        import numpy as np
        ips = self._pod_ips(pods)
        n = len(ips)
        if n == 0 or not services:
            return []
        index = {pod: k for k, pod in reversed(list(enumerate(pods)))}
        s = np.arange(n, dtype=np.uint32) if sources is None else np.array([index[p] for p in sources], np.uint32)
        t = np.arange(n, dtype=np.uint32) if targets is None else np.array([index[p] for p in targets], np.uint32)
        _, hop, _ = self._closure(ips, services, max_hops, host, True)
        cnt = self._paths(hop, n, np.repeat(s, t.size), np.tile(t, s.size), host, via=True)
        order = np.argsort(-cnt.astype(np.int64), kind="stable")
        return [(pods[int(k)], int(cnt[k])) for k in order if cnt[k]]

    def debug_reach_groups_host(self, matrix, n_src, n_dst, src_group, dst_group, n_src_groups, n_dst_groups, packed=True):
        """TESTS ONLY: pg_reach_groups's per-word code run on the host (pg_debug_reach_groups_host)
        over a numpy array of packed words [n_svc, n_src, row_words(n_dst)]. -> (counts u64 [n_svc,
        n_sg, n_dg, 4], status words u32 [n_svc, n_sg, row_words(n_dg)] or None); the outputs are
        pre-filled with 0xFF.."""
        import numpy as np
        from . import device as D
        m = np.ascontiguousarray(matrix, dtype=np.uint32)
        n_svc = m.shape[0] if m.ndim == 3 else m.size // max(1, n_src * lib.pg_reach_row_words(n_dst))
        counts = np.full((n_svc, n_src_groups, n_dst_groups, 4), 0xFFFFFFFFFFFFFFFF, np.uint64)
        status = np.full((n_svc, n_src_groups, lib.pg_reach_row_words(n_dst_groups)), 0xFFFFFFFF, np.uint32) if packed else None
        if counts.size == 0:
            return counts, status
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        spec, keep = D.groups_spec(m.ctypes.data if m.size else None, n_svc, n_src, n_dst, src_group, dst_group,
                                   n_src_groups, n_dst_groups)
        self._ck(lib.pg_debug_reach_groups_host(self.h, C.byref(spec), p(counts), p(status) if packed else None))
        del keep
        return counts, status

    def debug_reach_groups_plan(self, n_dst):
        """TESTS ONLY: how pg_reach_groups cuts rows of n_dst cells (pg_debug_reach_groups_plan) ->
        {tile_words, chunk_rows}"""
        t, c = C.c_uint32(), C.c_uint32()
        self._ck(lib.pg_debug_reach_groups_plan(self.h, int(n_dst), C.byref(t), C.byref(c)))
        return {"tile_words": t.value, "chunk_rows": c.value}

    def _groups(self, src_groups, dst_groups, services, host):
        """one pg_reach_matrix over the groups' pods, listed once per group they are in, and one
        pg_reach_groups -> (counts u64 [n_svc, n_sg, n_dg, 4], status words [n_svc, n_sg,
        row_words(n_dg)]), device tensors or with ``host`` numpy arrays"""
        import numpy as np
        from . import device as D
        src = [ip for pods in src_groups.values() for ip in self._pod_ips(pods)]
        dst = [ip for pods in dst_groups.values() for ip in self._pod_ips(pods)]
        sg = np.repeat(np.arange(len(src_groups), dtype=np.uint32), [len(p) for p in src_groups.values()])
        dg = np.repeat(np.arange(len(dst_groups), dtype=np.uint32), [len(p) for p in dst_groups.values()])
        if host:
            m = self.debug_reach_matrix_host(src, dst, services, words=False)
            return self.debug_reach_groups_host(m, len(src), len(dst), sg, dg, len(src_groups), len(dst_groups))
        m = D.reach_matrix(self, src, dst, services)
        return D.reach_groups(self, m, len(src), len(dst), sg, dg, len(src_groups), len(dst_groups), packed=True)

    def reachability_groups(self, src_groups, dst_groups, services, host=False):
        """Which groups reach which, and how fully: ``src_groups`` / ``dst_groups`` are ordered mappings
        from a name (a namespace, a deployment, a label set) to a list of pods; a pod may be in several
        groups. One pg_reach_matrix and one pg_reach_groups. -> (counts uint64 [n_svc, n_sg, n_dg, 4]:
        the (src pod, dst pod) cells of every (service, src group, dst group) by ConnAction, status
        uint8 [n_svc, n_sg, n_dg]: GROUPS_NONE / SOME / ALL of them ALLOW, or GROUPS_EMPTY) in the
        mappings' order. Pods and services as in reachability. ``host``: TESTS ONLY, the host twins."""
        import numpy as np
        from . import device as D
        n_sg, n_dg = len(src_groups), len(dst_groups)
        if not services or not n_sg or not n_dg:
            return np.zeros((len(services), n_sg, n_dg, 4), np.uint64), np.zeros((len(services), n_sg, n_dg), np.uint8)
        counts, status = self._groups(src_groups, dst_groups, services, host)
        if not host:
            counts = counts.cpu().numpy().view(np.uint64)
        return counts, D.unpack_groups(status, n_dg)

    def reachability_groups_diff(self, baseline, src_groups, dst_groups, services, host=False):
        """Which group pairs a policy change moved: the (service, src group, dst group) whose status
        under this engine differs from that under ``baseline`` (another Engine on the same device), by
        two pg_reach_matrix calls, two pg_reach_groups calls and one pg_reach_diff over the summaries.
        -> [(service index, src group, dst group, status before, after), ...] in (service, src group,
        dst group) order with the names as given. ``host``: TESTS ONLY, the host twins."""
        from . import device as D
        n_sg, n_dg = len(src_groups), len(dst_groups)
        if not services or not n_sg or not n_dg:
            return []
        _, b = baseline._groups(src_groups, dst_groups, services, host)
        _, a = self._groups(src_groups, dst_groups, services, host)
        if host:
            k, changes, _, _ = self.debug_reach_diff_host(b, a, n_dg, row_changes=False)
            changes = changes[:k]
        else:
            _, changes, _, _ = D.reach_diff(self, b, a, n_dg)
        row, col, cb, ca = D.unpack_changes(changes)
        sn, dn = list(src_groups), list(dst_groups)
        return [(int(r) // n_sg, sn[int(r) % n_sg], dn[int(j)], int(x), int(y)) for r, j, x, y in zip(row, col, cb, ca)]

    def debug_reach_classes_host(self, matrix, n_svc, n_src, n_dst, src=True, dst=True, reps=True, quotient=True):
        """TESTS ONLY: pg_reach_classes's per-word code, signatures, rounds and plan run on the host
        (pg_debug_reach_classes_host) over a numpy array of packed words [n_svc, n_src,
        row_words(n_dst)]. -> (src_class u32 [n_src], dst_class u32 [n_dst], src_rep u32 [n_src_classes],
        dst_rep u32 [n_dst_classes], quotient words u32 [n_svc, n_src_classes, row_words(n_dst_classes)],
        {n_src_classes, n_dst_classes, rounds}), None for what was not asked for."""
        import numpy as np
        from . import device as D
        m = np.ascontiguousarray(matrix, dtype=np.uint32)
        quotient = quotient and src and dst
        new = lambda n: np.full(n, 0xFFFFFFFF, np.uint32)
        sc, dc = new(n_src) if src else None, new(n_dst) if dst else None
        sr, dr = new(n_src) if src and reps else None, new(n_dst) if dst and reps else None
        q = new(m.size) if quotient else None
        res = _capi.pg_reach_classes_result()
        if m.size:
            p = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None and x.size else None
            spec = _capi.pg_reach_classes_spec(m.ctypes.data, int(n_svc), int(n_src), int(n_dst))
            self._ck(lib.pg_debug_reach_classes_host(self.h, C.byref(spec), p(sc), p(dc), p(sr), p(dr), p(q), C.byref(res)))
        n_sc, n_dc = res.n_src_classes, res.n_dst_classes
        rwq = lib.pg_reach_row_words(n_dc)
        return (sc, dc, None if sr is None else sr[:n_sc], None if dr is None else dr[:n_dc],
                None if q is None else q[:n_svc * n_sc * rwq].reshape(n_svc, n_sc, rwq), D.classes_result(res))

    def debug_reach_classes_plan(self, n_dst):
        """TESTS ONLY: how the column passes of pg_reach_classes cut rows of n_dst cells
        (pg_debug_reach_classes_plan) -> {tile_words, chunk_rows, check_rows}"""
        t, c, k = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._ck(lib.pg_debug_reach_classes_plan(self.h, int(n_dst), C.byref(t), C.byref(c), C.byref(k)))
        return {"tile_words": t.value, "chunk_rows": c.value, "check_rows": k.value}

    def reachability_classes(self, src_pods, dst_pods, services, host=False):
        """Which pods the policy treats as one role: the src pods with identical rows and the dst pods
        with identical columns over all of ``services``, by one pg_reach_matrix and one
        pg_reach_classes. -> (src classes, dst classes, codes): two lists of pod lists, the classes in
        the order of their first member and every class's members in list order (a pod listed twice
        is there twice), and the ConnActions uint8 [n_svc, n_src_classes, n_dst_classes] of the
        classes' first members. Pods and services as in reachability. ``host``: TESTS ONLY, the host
        twins."""
        import numpy as np
        from . import device as D
        src, dst = self._pod_ips(src_pods), self._pod_ips(dst_pods)
        n_svc, n_src, n_dst = len(services), len(src), len(dst)
        if not n_svc or not n_src or not n_dst:
            # (no cell tells two end points apart: each side is one class)
            one = lambda pods: [list(pods)] if len(pods) else []
            return one(src_pods), one(dst_pods), np.zeros((n_svc, min(n_src, 1), min(n_dst, 1)), np.uint8)
        if host:
            m = self.debug_reach_matrix_host(src, dst, services, words=False)
            sc, dc, _, _, q, res = self.debug_reach_classes_host(m, n_svc, n_src, n_dst, reps=False)
        else:
            m = D.reach_matrix(self, src, dst, services)
            sc, dc, _, _, q, res = D.reach_classes(self, m, n_svc, n_src, n_dst, quotient=True)
            sc, dc = sc.cpu().numpy(), dc.cpu().numpy()
        n_sc, n_dc = res["n_src_classes"], res["n_dst_classes"]
        members = lambda cls, pods, n: [[pods[k] for k in np.flatnonzero(cls == c)] for c in range(n)]
        return members(sc, src_pods, n_sc), members(dc, dst_pods, n_dc), D.unpack_reach(q, n_svc, n_sc, n_dc)

    def debug_reach_zones_host(self, closure, n, reps=True, sizes=True, counts=True, dag=True):
        """TESTS ONLY: pg_reach_zones's per-word code and plan run on the host (pg_debug_reach_zones_host)
        over a numpy array of packed words [n, row_words(n)]. -> (zone u32 [n], rep, size, reaches,
        reached_by u32 [n_zones], dag words u32 [n_zones, row_words(n_zones)], {n_zones, n_cyclic, n_multi,
        largest, n_broken}), None for what was not asked for (``dag`` takes the representatives)."""
        import numpy as np
        from . import device as D
        m = np.ascontiguousarray(closure, dtype=np.uint32)
        reps = reps or dag
        new = lambda k: np.full(k, 0xFFFFFFFF, np.uint32)
        zone = new(n)
        rep, size = new(n) if reps else None, new(n) if sizes else None
        out, by = (new(n), new(n)) if counts else (None, None)
        graph = new(m.size) if dag else None
        res = _capi.pg_reach_zones_result()
        if n:
            p = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None
            spec = _capi.pg_reach_zones_spec(m.ctypes.data, int(n))
            self._ck(lib.pg_debug_reach_zones_host(self.h, C.byref(spec), p(zone), p(rep), p(size), p(out), p(by), p(graph),
                                                   C.byref(res)))
        nz = res.n_zones
        rwz = lib.pg_reach_row_words(nz)
        cut = lambda x: None if x is None else x[:nz]
        return (zone, cut(rep), cut(size), cut(out), cut(by), None if graph is None else graph[:nz * rwz].reshape(nz, rwz),
                D.zones_result(res))

    def debug_reach_zones_plan(self, n):
        """TESTS ONLY: how pg_reach_zones over n end points is cut (pg_debug_reach_zones_plan) ->
        {tile_rows, tile_cols, row_tiles, col_tiles, bits_grid, label_rows, label_grid, dag_grid}"""
        p = _capi.pg_reach_zones_plan()
        self._ck(lib.pg_debug_reach_zones_plan(self.h, int(n), C.byref(p)))
        return {name: getattr(p, name) for name, _ in p._fields_}

    def debug_reach_dominators_host(self, matrix, n, entry, svc_select=None, dom=True, idom=True, cut=True):
        """TESTS ONLY: pg_reach_dominators's per-word code and plan run on the host
        (pg_debug_reach_dominators_host) over a numpy array of packed words [n_svc, n, row_words(n)]. ->
        (dom words u32 [n, row_words(n)], idom u16 [n], cut u32 [n], {n_reached, n_chokes, top, top_cut,
        depth, rounds}), None for what was not asked for; the outputs are pre-filled with 0xFF.."""
        import numpy as np
        from . import device as D
        m = np.ascontiguousarray(matrix, dtype=np.uint32)
        rw = lib.pg_reach_row_words(n)
        n_svc = m.size // (n * rw) if n else 1
        d = np.full((n, rw), 0xFFFFFFFF, np.uint32) if dom else None
        i = np.full(n, 0xFFFF, np.uint16) if idom else None
        c = np.full(n, 0xFFFFFFFF, np.uint32) if cut else None
        res = _capi.pg_reach_dominators_result()
        p = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None and x.size else None
        spec, keep = D.dominators_spec(m.ctypes.data if m.size else None, n, n_svc, entry, svc_select)
        self._ck(lib.pg_debug_reach_dominators_host(self.h, C.byref(spec), p(d), p(i), p(c), C.byref(res)))
        del keep
        return d, i, c, D.dominators_result(res)

    def debug_reach_dominators_plan(self, n):
        """TESTS ONLY: how pg_reach_dominators over n end points is cut (pg_debug_reach_dominators_plan) ->
        {lane_words, tile_rows, tile_cols, row_tiles, col_tiles, round_grid, t_rows, t_cols, t_row_tiles,
        t_col_tiles, t_grid, cut_rows, cut_cols, cut_row_tiles, cut_col_tiles, cut_grid, finish_grid}"""
        p = _capi.pg_reach_dominators_plan()
        self._ck(lib.pg_debug_reach_dominators_plan(self.h, int(n), C.byref(p)))
        return {name: getattr(p, name) for name, _ in p._fields_}

    def reachability_dominators(self, pods, services, entry_pods, host=False):
        """Incident response: the attacker holds ``entry_pods``; which single pod, if quarantined, cuts
        them off from the most of ``pods``, and which pod stands last before each pod on every route over
        ``services``? The exact choke points, where reachability_chokepoints counts one shortest path per
        pair. One pg_reach_matrix over pods x pods and one pg_reach_dominators. -> (chokes, idom,
        result): the pods outside the foothold whose removal alone cuts the attacker off from at least one
        other pod, as [(pod, cut), ...] by cut descending (ties in list order); per listed pod its
        immediate dominator -- the last pod every route to it crosses -- or None for a pod of the foothold,
        a pod that is not reached and a pod with no choke point before it; and {n_reached, n_chokes, top,
        top_cut, depth, rounds} with ``top`` as a pod (None when there is no choke point). Every entry pod
        has to be among ``pods``. Pods and services as in reachability. ``host``: TESTS ONLY, the host
        twins."""
        import numpy as np
        from . import device as D
        ips = self._pod_ips(pods)
        n = len(ips)
        entry = []
        for e, ip in zip(entry_pods, self._pod_ips(entry_pods)):
            at = [k for k in range(n) if ips[k] == ip]
            if not at:
                raise ValueError("entry pod %s is not among the pods" % (e,))
            entry += at
        if n == 0 or not services:
            # (no edge: the foothold reaches nothing but itself)
            return [], [None] * n, {"n_reached": len(set(entry)), "n_chokes": 0, "top": None, "top_cut": 0, "depth": 0,
                                    "rounds": 0}
        if host:
            m = self.debug_reach_matrix_host(ips, ips, services, words=False)
            _, idom, cut, res = self.debug_reach_dominators_host(m, n, entry, dom=False)
        else:
            m = D.reach_matrix(self, ips, ips, services)
            _, idom, cut, res = D.reach_dominators(self, m, n, len(services), entry, idom=True, cut=True)
            idom, cut = idom.cpu().numpy().view(np.uint16), cut.cpu().numpy().view(np.uint32)
        held = set(entry)
        order = sorted((k for k in range(n) if cut[k] and k not in held), key=lambda k: (-int(cut[k]), k))
        res = dict(res, top=None if res["n_chokes"] == 0 else pods[res["top"]])
        return ([(pods[k], int(cut[k])) for k in order], [None if k == D.NO_IDOM else pods[int(k)] for k in idom], res)

    def debug_reach_cut_host(self, matrix, n, entry, target, max_cut=16, svc_select=None, cut=True, paths=True):
        """TESTS ONLY: pg_reach_cut's per-word code and plan run on the host (pg_debug_reach_cut_host) over a
        numpy array of packed words [n_svc, n, row_words(n)]. -> (cut u8 [n], prev u16 [n], next u16 [n],
        {separable, capped, n_direct, cut_size, n_paths, near_reach, far_reach, levels, reroutes}), None for
        what was not asked for; the outputs are pre-filled with 0xEE.."""
        import numpy as np
        from . import device as D
        m = np.ascontiguousarray(matrix, dtype=np.uint32)
        rw = lib.pg_reach_row_words(n)
        n_svc = m.size // (n * rw) if n else 1
        c = np.full(n, 0xEE, np.uint8) if cut else None
        pv = np.full(n, 0xEEEE, np.uint16) if paths else None
        nx = np.full(n, 0xEEEE, np.uint16) if paths else None
        res = _capi.pg_reach_cut_result()
        p = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None and x.size else None
        spec, keep = D.cut_spec(m.ctypes.data if m.size else None, n, n_svc, entry, target, max_cut, svc_select)
        self._ck(lib.pg_debug_reach_cut_host(self.h, C.byref(spec), p(c), p(pv), p(nx), C.byref(res)))
        del keep
        return c, pv, nx, D.cut_result(res)

    def debug_reach_cut_plan(self, n):
        """TESTS ONLY: how pg_reach_cut over n end points is cut (pg_debug_reach_cut_plan) -> {lane_words,
        level_block, group_nodes, row_steps, level_grid, t_rows, t_cols, t_row_tiles, t_col_tiles, t_grid,
        finish_block, finish_grid}"""
        p = _capi.pg_reach_cut_plan()
        self._ck(lib.pg_debug_reach_cut_plan(self.h, int(n), C.byref(p)))
        return {name: getattr(p, name) for name, _ in p._fields_}

    def reachability_cut(self, pods, services, entry_pods, target_pods, max_cut=16, host=False):
        """Incident response past the single choke point: the attacker holds ``entry_pods`` and wants
        ``target_pods``; what is the smallest set of other pods among ``pods`` to quarantine so that no route
        over ``services`` is left, and how many independent routes are there today? One pg_reach_matrix over
        pods x pods and one pg_reach_cut. -> (near, far, routes, result): the minimum cut closest to the
        attacker and the one closest to the targets as lists of pods in list order (both [] when the input
        is inseparable or the search was capped at ``max_cut`` + 1 routes), the witness routes -- pairwise
        sharing no pod outside the two sets -- as lists of pods from an entry to a target, and {separable,
        capped, n_direct, cut_size, n_paths, near_reach, far_reach, levels, reroutes} with cut_size None
        when there is none to report. Every entry and target pod has to be among ``pods``. Pods and services
        as in reachability. ``host``: TESTS ONLY, the host twins."""
        import numpy as np
        from . import device as D
        ips = self._pod_ips(pods)
        n = len(ips)

        def ids(names, what):
            out = []
            for e, ip in zip(names, self._pod_ips(names)):
                at = [k for k in range(n) if ips[k] == ip]
                if not at:
                    raise ValueError("%s pod %s is not among the pods" % (what, e))
                out += at
            return out
        entry, target = ids(entry_pods, "entry"), ids(target_pods, "target")
        if n == 0 or not services:
            # (no edge: only a pod on both sides joins them)
            direct = len(set(entry) & set(target))
            return [], [], [], {"separable": int(not direct), "capped": 0, "n_direct": direct, "cut_size": None if direct else 0,
                                "n_paths": 0, "near_reach": 0 if direct else len(set(entry)),
                                "far_reach": 0 if direct else len(set(entry)), "levels": 0, "reroutes": 0}
        if host:
            m = self.debug_reach_matrix_host(ips, ips, services, words=False)
            cut, prev, nxt, res = self.debug_reach_cut_host(m, n, entry, target, max_cut)
        else:
            m = D.reach_matrix(self, ips, ips, services)
            cut, prev, nxt, res = D.reach_cut(self, m, n, len(services), entry, target, max_cut, cut=True, paths=True)
            cut, prev, nxt = cut.cpu().numpy(), prev.cpu().numpy().view(np.uint16), nxt.cpu().numpy().view(np.uint16)
        res = dict(res, cut_size=None if res["cut_size"] == D.NO_CUT else res["cut_size"])
        return ([pods[k] for k in range(n) if cut[k] & _capi.CUT_NEAR], [pods[k] for k in range(n) if cut[k] & _capi.CUT_FAR],
                [[pods[k] for k in route] for route in D.cut_routes(prev, nxt, entry)], res)

    def debug_reach_cost_host(self, matrix, n, src, weight, max_cost=0, svc_select=None, cost=True, pred=True, len=True, via=True):
        """TESTS ONLY: pg_reach_cost's per-word code run on the host (pg_debug_reach_cost_host) over a numpy
        array of packed words [n_svc, n, row_words(n)]. -> (cost u32 [n_src, n], pred u16 [n_src, n], len u16
        [n_src, n], via u32 [n], {n_reached, n_via, max_cost, longest}), None for what was not asked for; the
        outputs are pre-filled with 0xEE.."""
        import numpy as np
        from . import device as D
        m = np.ascontiguousarray(matrix, dtype=np.uint32)
        rw = lib.pg_reach_row_words(n)
        n_svc = m.size // (n * rw) if n else 1
        spec, keep = D.cost_spec(m.ctypes.data if m.size else None, n, n_svc, src, weight, max_cost, svc_select)
        c = np.full((spec.n_src, n), 0xEEEEEEEE, np.uint32) if cost else None
        pd = np.full((spec.n_src, n), 0xEEEE, np.uint16) if pred else None
        ln = np.full((spec.n_src, n), 0xEEEE, np.uint16) if len else None
        v = np.full(n, 0xEEEEEEEE, np.uint32) if via else None
        res = _capi.pg_reach_cost_result()
        p = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None and x.size else None
        self._ck(lib.pg_debug_reach_cost_host(self.h, C.byref(spec), p(c), p(pd), p(ln), p(v), C.byref(res)))
        del keep
        return c, pd, ln, v, D.cost_result(res)

    def debug_reach_cost_plan(self, n):
        """TESTS ONLY: how pg_reach_cost over n end points is laid out under this engine's "cost_lds_bytes"
        (pg_debug_reach_cost_plan) -> {lane_words, block, lds_bytes, row_in_lds, weights_in_lds, t_rows,
        t_cols, t_row_tiles, t_col_tiles, t_grid}"""
        p = _capi.pg_reach_cost_plan()
        self._ck(lib.pg_debug_reach_cost_plan(self.h, int(n), C.byref(p)))
        return {name: getattr(p, name) for name, _ in p._fields_}

    def reachability_cost(self, pods, services, src_pods, weights, max_cost=0, host=False):
        """Budgeted blast radius: the attacker holds each of ``src_pods`` in turn and taking a pod costs
        ``weights[pod]`` (a mapping pod -> 1..65535, a pod it does not name costs 1); what is the cheapest
        route to every pod of ``pods`` over ``services``, and which pods do most cheapest routes cross? With
        ``max_cost`` != 0 only pods within that budget are reached. One pg_reach_matrix over pods x pods and
        one pg_reach_cost. -> (routes, chokes, result): per source pod a dict {pod: (cost, [source, .., pod])}
        of the reached pods (the source itself only when a cycle leads back to it); the pods that are an
        intermediate of some route as [(pod, routes), ...] by routes descending (ties in list order); and
        {n_reached, n_via, max_cost, longest}. Every source pod has to be among ``pods``. Pods and services as
        in reachability. ``host``: TESTS ONLY, the host twins."""
        import numpy as np
        from . import device as D
        ips = self._pod_ips(pods)
        n = len(ips)
        src = []
        for e, ip in zip(src_pods, self._pod_ips(src_pods)):
            at = [k for k in range(n) if ips[k] == ip]
            if not at:
                raise ValueError("source pod %s is not among the pods" % (e,))
            src.append(at[0])
        if n == 0 or not services or not src:
            # (no edge or no source: nothing is reached)
            return [{} for _ in src], [], {"n_reached": 0, "n_via": 0, "max_cost": 0, "longest": 0}
        w = [int(weights.get(p, 1)) for p in pods]
        if host:
            m = self.debug_reach_matrix_host(ips, ips, services, words=False)
            cost, pred, _, via, res = self.debug_reach_cost_host(m, n, src, w, max_cost, len=False)
        else:
            m = D.reach_matrix(self, ips, ips, services)
            cost, pred, _, via, res = D.reach_cost(self, m, n, len(services), src, w, max_cost, pred=True, via=True)
            cost, pred, via = cost.cpu().numpy().view(np.uint32), pred.cpu().numpy().view(np.uint16), via.cpu().numpy().view(np.uint32)
        routes = []
        for q, s in enumerate(src):
            found = {}
            for v in range(n):
                if cost[q, v] == D.NO_COST:
                    continue
                back = [v]
                while int(pred[q, back[-1]]) != s and len(back) <= n:
                    back.append(int(pred[q, back[-1]]))
                found[pods[v]] = (int(cost[q, v]), [pods[k] for k in [s] + back[::-1]])
            routes.append(found)
        order = sorted((k for k in range(n) if via[k]), key=lambda k: (-int(via[k]), k))
        return routes, [(pods[k], int(via[k])) for k in order], res

    def reach_observed(self, src_ips, dst_ips, services, batch, **kw):
        """A flow log as a reach matrix on the GPU: device.reach_observed on this engine (which only names
        the device: the call reads no table)."""
        from . import device as D
        return D.reach_observed(self, src_ips, dst_ips, services, batch, **kw)

    def debug_reach_observed_host(self, src_ips, dst_ips, services, flows, flags=0, into=None, flow=True, svc_flows=True):
        """TESTS ONLY: pg_reach_observed's tables and per-flow code run on the host
        (pg_debug_reach_observed_host). flows: numpy arrays (src, dst, src port or None, dst port, proto);
        flags: PG_OBSERVED_*; into: packed words that ACCUMULATE ORs into. -> (packed u32 [n_svc, n_src,
        row_words], flow statuses u8 [n], flows per service u64 [n_svc], {n_matched, .., n_cells}), None
        for what was not asked for."""
        import numpy as np
        from . import device as D
        spec, keep = D.observed_spec(src_ips, dst_ips, services, flags)
        src, dst, sport, dport, proto = flows
        arrs = [np.ascontiguousarray(src, np.uint32), np.ascontiguousarray(dst, np.uint32),
                None if sport is None else np.ascontiguousarray(sport, np.uint16), np.ascontiguousarray(dport, np.uint16),
                np.ascontiguousarray(proto, np.uint8)]
        n = len(arrs[0])
        soa = _capi.pg_tuple_soa(*[None if a is None else a.ctypes.data for a in arrs])
        shape = (len(services), spec.n_src, lib.pg_reach_row_words(spec.n_dst))
        packed = np.full(shape, 0xFFFFFFFF, np.uint32) if into is None else np.ascontiguousarray(into, np.uint32).reshape(shape).copy()
        out_flow = np.full(n, 0xFF, np.uint8) if flow else None
        counts = np.full(len(services), 0xFFFFFFFFFFFFFFFF, np.uint64) if svc_flows else None
        res = _capi.pg_reach_observed_result()
        p = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None
        self._ck(lib.pg_debug_reach_observed_host(self.h, C.byref(spec), C.byref(soa), n,
                                                  p(packed) if packed.size else C.c_void_p(16), p(out_flow), p(counts),
                                                  C.byref(res)))
        del keep
        return packed, out_flow, counts, D.observed_result(res)

    def debug_reach_observed_plan(self, n_src, n_dst, n_svc):
        """TESTS ONLY: how pg_reach_observed over lists of these lengths is laid out under this context's
        knobs (pg_debug_reach_observed_plan) -> {src_cap, dst_cap, src_in_lds, dst_in_lds, svc_bytes,
        lds_bytes, block, vec_flows, grid}"""
        p = _capi.pg_reach_observed_plan()
        self._ck(lib.pg_debug_reach_observed_plan(self.h, int(n_src), int(n_dst), int(n_svc), C.byref(p)))
        return {name: getattr(p, name) for name, _ in p._fields_}

    def debug_reach_observed_probe(self, ip_list, ips):
        """TESTS ONLY: where the address table pg_reach_observed builds over ``ip_list`` finds each address
        (pg_debug_reach_observed_probe) -> (probe steps u32 [n], start slot u32 [n], the table's capacity)"""
        import numpy as np
        ip_list = np.ascontiguousarray(ip_list, dtype=np.uint32)
        ips = np.ascontiguousarray(ips, dtype=np.uint32)
        steps, slot, cap = np.zeros(len(ips), np.uint32), np.zeros(len(ips), np.uint32), C.c_uint32()
        p = lambda x: x.ctypes.data_as(C.c_void_p) if len(x) else None
        self._ck(lib.pg_debug_reach_observed_probe(self.h, p(ip_list), len(ip_list), p(ips), len(ips), p(steps), p(slot),
                                                   C.byref(cap)))
        return steps, slot, cap.value

    def _zones(self, ips, services, host, **kw):
        """one _closure (max_hops 0) and one pg_reach_zones over it -> (closure words, reach_zones's
        tuple), device tensors or with ``host`` numpy arrays"""
        from . import device as D
        packed, _, _ = self._closure(ips, services, 0, host, False)
        if host:
            return packed, self.debug_reach_zones_host(packed, len(ips), **kw)
        return packed, D.reach_zones(self, packed, len(ips), **kw)

    def reachability_zones(self, pods, services, host=False):
        """Lateral-movement zones: the pods that can all reach each other in any number of hops over
        ``services`` (the strongly connected components of the ALLOW graph), and how the zones sit to one
        another, by one pg_reach_matrix over pods x pods, one pg_reach_closure and one pg_reach_zones. ->
        (zones, reaches, reached_by, graph): the zones as lists of pods, in the order of their first member
        and every zone's members in list order (a pod that lies on no cycle is a zone of its own); per
        zone the number of listed pods it reaches (its blast radius) and that reach it (its exposure),
        uint32 arrays [n_zones]; and the bool array [n_zones, n_zones], graph[a, b] = zone a reaches zone b
        (graph[z, z]: the zone's members lie on a cycle). Pods and services as in reachability. ``host``:
        TESTS ONLY, the host twins."""
        import numpy as np
        from . import device as D
        ips = self._pod_ips(pods)
        n = len(ips)
        if n == 0 or not services:
            # (no edge: every pod is a zone that reaches nothing)
            return [[p] for p in pods], np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros((n, n), bool)
        _, (zone, _, _, out, by, graph, res) = self._zones(ips, services, host, reps=False, sizes=False, counts=True, dag=True)
        if not host:
            zone, out, by = (t.cpu().numpy().view(np.uint32) for t in (zone, out, by))
        nz = res["n_zones"]
        members = [[pods[k] for k in np.flatnonzero(zone == z)] for z in range(nz)]
        return members, out, by, D.unpack_closure(graph, nz)

    def reachability_zones_diff(self, baseline, pods, services, host=False):
        """Which zones a policy change connected or cut: the zones are those under ``baseline`` (another
        Engine on the same device); the closure under the baseline and the closure under this engine are
        each summed into (zone, zone) pairs by pg_reach_groups, and one pg_reach_diff over the two
        summaries lists the pairs whose status moved. -> [(src zone, dst zone, status before, after), ...]
        in (src zone, dst zone) order, the zones as lists of pods as reachability_zones gives them for the
        baseline; the status is GROUPS_NONE / SOME / ALL of the zone pair's (src pod, dst pod) cells
        reachable (before, a pair is NONE or ALL; after, SOME says that only a part of the two zones got
        connected or stayed so). At most 4096 zones. ``host``: TESTS ONLY, the host twins."""
        import numpy as np
        from . import device as D
        ips = self._pod_ips(pods)
        n = len(ips)
        if n == 0 or not services:
            return []
        b, (zone, _, _, _, _, _, res) = baseline._zones(ips, services, host, reps=False, sizes=False, counts=False, dag=False)
        a, _, _ = self._closure(ips, services, 0, host, False)
        nz = res["n_zones"]
        if host:
            sb, sa = (self.debug_reach_groups_host(m.reshape(1, n, -1), n, n, zone, zone, nz, nz)[1] for m in (b, a))
            k, changes, _, _ = self.debug_reach_diff_host(sb, sa, nz, row_changes=False)
            changes = changes[:k]
        else:
            zone = zone.cpu().numpy().view(np.uint32)
            sb, sa = (D.reach_groups(self, m.reshape(1, n, -1), n, n, zone, zone, nz, nz, packed=True)[1] for m in (b, a))
            _, changes, _, _ = D.reach_diff(self, sb, sa, nz)
        members = [[pods[k] for k in np.flatnonzero(zone == z)] for z in range(nz)]
        row, col, cb, ca = D.unpack_changes(changes)
        return [(members[int(r)], members[int(j)], int(x), int(y)) for r, j, x, y in zip(row, col, cb, ca)]

    def debug_reach_rules_host(self, src_ips, dst_ips, services, weights=None, evals=True, cells=True, node=True,
                               n_slots=None):
        """TESTS ONLY: pg_reach_rules's per-word code, sink, windows and flushes run on the host
        (pg_debug_reach_rules_host). -> (evals u64 [n_slots], cells u64 [n_slots, 4], result dict), None
        for a histogram that was not asked for; the outputs are pre-filled with ones in every bit."""
        import numpy as np
        from . import device as D
        n = self.num_counter_slots() if n_slots is None else n_slots
        spec, keep = D.rules_spec(src_ips, dst_ips, services, weights, n)
        ev = np.full(n, 0xFFFFFFFFFFFFFFFF, np.uint64) if evals else None
        ce = np.full((n, 4), 0xFFFFFFFFFFFFFFFF, np.uint64) if cells else None
        res = _capi.pg_reach_rules_result()
        p = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None
        self._ck(lib.pg_debug_reach_rules_host(self.h, C.byref(spec), p(ev), p(ce), C.byref(res), int(node)))
        del keep
        return ev, ce, D.rules_result(res)

    def debug_reach_rules_plan(self, n_slots, n_tail=2, evals=True, cells=True, max_weight=65536, resident=False):
        """TESTS ONLY: the launch plan of pg_reach_rules (pg_debug_reach_rules_plan) -> {block, evals_cells,
        evals_base, cells_cells, cells_base, flush_words, lds_bytes}, and with ``resident`` (needs the
        GPU) the workgroups the device holds at once"""
        plan, res = _capi.pg_reach_rules_plan(), C.c_uint32()
        self._ck(lib.pg_debug_reach_rules_plan(self.h, int(n_slots), int(n_tail), int(evals), int(cells), int(max_weight),
                                               C.byref(plan), C.byref(res) if resident else None))
        out = {k: getattr(plan, k) for k, _ in _capi.pg_reach_rules_plan._fields_}
        if resident:
            out["resident"] = res.value
        return out

    def _coverage(self, src, dst, services, weights, host, max_services=4096):
        """(evals [n_slots], cells [n_slots, 4]) as Python-int numpy arrays of one product, by as many
        pg_reach_rules calls as ``max_services`` asks for, summed (on the device unless ``host``)"""
        import numpy as np
        from . import device as D
        n = self.num_counter_slots()
        ev, ce = None, None
        for k0 in range(0, max(len(services), 1), max_services):
            part = services[k0:k0 + max_services]
            w = None if weights is None else weights[k0:k0 + max_services]
            if host:
                e1, c1, _ = self.debug_reach_rules_host(src, dst, part, w)
            else:
                e1, c1, _ = D.reach_rules(self, src, dst, part, w)
            ev, ce = (e1, c1) if ev is None else (ev + e1, ce + c1)
        if not host:
            ev, ce = ev.cpu().numpy(), ce.cpu().numpy()
        return ev.astype(np.uint64).reshape(n), ce.astype(np.uint64).reshape(n, 4)

    def _coverage_report(self, ev, ce):
        n = len(ev)
        row = lambda s, k: (k, int(ev[s]), [int(x) for x in ce[s]])
        acls, dead = {}, []
        for name in self.ACLNames():
            tid = lib.pg_table_id(self.h, _b(name))
            if tid < 0:   # (an ACL no table was compiled for)
                continue
            base, n_rules, dflt = self.table_info(tid)
            acls[name] = [row(base + k, k) for k in range(n_rules)] + [row(dflt, -1)]
            dead += [(name, k) for k in range(n_rules) if not ev[base + k]]
        return {"acls": acls, "no_acl": row(n - 2, None)[1:], "unresolved": row(n - 1, None)[1:], "dead_rules": dead}

    def rule_coverage(self, src_pods, dst_pods, services, weights=None, host=False):
        """Which rules do any work over these pods and services, and which are dead or shadowed: by one
        pg_reach_rules call, without the reach matrix. -> {"acls": {ACL name: [(rule index, evals,
        cells[4])]}, the rules in order and last (-1, ...) for the ACL's default deny; "no_acl" and
        "unresolved": (evals, cells[4]) of the evaluations of an interface without an ACL and of the pairs
        that fail before any; "dead_rules": [(ACL name, rule index)] that decided no evaluation}. evals:
        the evalACL evaluations the rule decided; cells[c]: the pairs whose final verdict it gave, by
        ConnAction. ``weights`` (per service, 0 .. 65536) count a service several times. Pods and
        services as in reachability. ``host``: TESTS ONLY, the host twin."""
        src, dst = self._pod_ips(src_pods), self._pod_ips(dst_pods)
        return self._coverage_report(*self._coverage(src, dst, list(services), weights, host))

    def rule_coverage_ports(self, src_pods, dst_pods, protocol, src_port=40000, host=False, max_services=4096):
        """rule_coverage over all 65,536 dst ports of TCP (0) or UDP (1): the services are the first
        ports of the elementary intervals (port_intervals) and the weights the interval lengths, so a
        pair costs K evaluations, not 65,536. More than ``max_services`` intervals (the call's 4096 at
        most) take several calls, summed on the device."""
        import numpy as np
        src, dst = self._pod_ips(src_pods), self._pod_ips(dst_pods)
        lo = self.port_intervals(protocol)
        lens = np.diff(np.append(lo.astype(np.int64), 65536)).astype(np.uint32)
        services = [(int(protocol), int(src_port), int(p)) for p in lo]
        return self._coverage_report(*self._coverage(src, dst, services, lens, host, min(int(max_services), 4096)))

    def debug_walk_stats(self, table_id, src, dst, dport, proto):
        """MEASUREMENT: per tuple, the loads a SINGLE launch on table_id makes of the table's
        structure (pg_debug_walk_stats) -> (lds_reads u32[n], mem_reads u32[n], launch STAGE)"""
        import numpy as np
        n = len(src)
        a = [np.ascontiguousarray(x, dt) for x, dt in ((src, np.uint32), (dst, np.uint32), (dport, np.uint16),
                                                       (proto, np.uint8))]
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        t = _capi.pg_tuple_soa(p(a[0]), p(a[1]), None, p(a[2]), p(a[3]))
        nl, nm, st = np.zeros(n, np.uint32), np.zeros(n, np.uint32), C.c_int()
        self._ck(lib.pg_debug_walk_stats(self.h, table_id, C.byref(t), n, nl.ctypes.data_as(C.POINTER(C.c_uint32)),
                                         nm.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(st)))
        return nl, nm, st.value

    def debug_launch_plan(self, table_id, counters=False):
        """TESTS ONLY: the launch a SINGLE classify on table_id makes under this context's knobs
        (pg_debug_launch_plan) -> {stage: the full k_classify STAGE code (4, 5, 1, 2, 0; dst-free
        tables 9, 10, 14, 8), stage_words, hist_cells}"""
        st, sw, hc = C.c_int(), C.c_uint32(), C.c_uint32()
        self._ck(lib.pg_debug_launch_plan(self.h, table_id, int(counters), C.byref(st), C.byref(sw), C.byref(hc)))
        return {"stage": st.value, "stage_words": sw.value, "hist_cells": hc.value}

    HIST_KINDS = ("none", "full32", "half16", "cache", "global", "window")

    def debug_node_launch_plan(self, mode, counters=False):
        """TESTS ONLY: the launch a PERPOD / CONN classify makes under this context's knobs
        (pg_debug_node_launch_plan) -> {path: "node" | "per-table", stage: the full k_classify STAGE
        code, stage_words, records_staged, hist_kind (HIST_KINDS), hist_cells, hist_bytes,
        defers_any}"""
        p = _capi.pg_node_launch_plan()
        self._ck(lib.pg_debug_node_launch_plan(self.h, mode, int(counters), C.byref(p)))
        return {"path": "node" if p.path else "per-table", "stage": p.stage_code, "stage_words": p.stage_words,
                "records_staged": bool(p.records_staged), "hist_kind": self.HIST_KINDS[p.hist_kind],
                "hist_cells": p.hist_cells, "hist_bytes": p.hist_bytes, "defers_any": bool(p.defers_any)}

    def node_stats(self):
        """node classifier size {ip_classes, key_classes, image_bytes, cross_bytes}, or None."""
        a, b = C.c_uint32(), C.c_uint32()
        c, d = C.c_uint64(), C.c_uint64()
        rc = lib.pg_node_stats(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d))
        if rc == -2:  # PG_ENOENT
            return None
        self._ck(rc)
        st = {"ip_classes": a.value, "key_classes": b.value, "image_bytes": c.value, "cross_bytes": d.value}
        base, common, pairs = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._ck(lib.pg_node_common_stats(self.h, C.byref(base), C.byref(common), C.byref(pairs)))
        st.update(base_image_bytes=base.value, common_row_pairs=common.value, table_ipclass_pairs=pairs.value)
        rb, inimg = C.c_uint64(), C.c_int()
        self._ck(lib.pg_node_list_stats(self.h, C.byref(rb), C.byref(inimg)))
        st.update(list_record_bytes=rb.value, list_records_in_image=bool(inimg.value))
        lt = C.c_uint64()
        self._ck(lib.pg_node_list_table_stats(self.h, C.byref(lt)))
        st.update(list_table_bytes=lt.value)
        u = self._ck(lib.pg_node_uniform(self.h))
        st.update(uniform=bool(u), wide_records=u == 2)
        return st

    def slot_of_rule(self, tid, idx):
        """counter slot of rule ``idx`` of table ``tid`` (idx -1: the table's default deny)."""
        base, n, dflt = self.table_info(tid)
        return base + idx if idx >= 0 else dflt

    # Connection* (aclengine_mock.go:273-420), testConnection evaluated on the GPU
    def connections(self, queries):
        """queries: list of (kind, a, b, proto, sport, dport) with kind in
        {"PodToPod", "PodToInternet", "InternetToPod"}; returns (ConnActions, slots)."""
        n = len(queries)
        arr = (_capi.pg_conn_query * max(1, n))()
        for i, (kind, a, b, proto, sport, dport) in enumerate(queries):
            q = arr[i]
            q.kind = {"PodToPod": 0, "PodToInternet": 1, "InternetToPod": 2}[kind]
            if q.kind == 0:
                (q.src_namespace, q.src_name), (q.dst_namespace, q.dst_name) = map(
                    lambda p: tuple(map(_b, _pod(p))), (a, b))
            elif q.kind == 1:
                q.src_namespace, q.src_name = map(_b, _pod(a))
                q.dst_ip = _b(b)
            else:
                q.src_ip = _b(a)
                q.dst_namespace, q.dst_name = map(_b, _pod(b))
            q.protocol, q.src_port, q.dst_port = proto, sport, dport
        out = (C.c_int32 * max(1, n))()
        slots = (C.c_uint32 * max(1, n))()
        self._ck(lib.pg_connections(self.h, arr, n, out, slots))
        return list(out[:n]), list(slots[:n])

    def ConnectionPodToPod(self, src_pod, dst_pod, protocol, src_port, dst_port):
        return self.connections([("PodToPod", src_pod, dst_pod, protocol, src_port, dst_port)])[0][0]

    def ConnectionPodToInternet(self, src_pod, dst_ip, protocol, src_port, dst_port):
        return self.connections([("PodToInternet", src_pod, dst_ip, protocol, src_port, dst_port)])[0][0]

    def ConnectionInternetToPod(self, src_ip, dst_pod, protocol, src_port, dst_port):
        return self.connections([("InternetToPod", src_ip, dst_pod, protocol, src_port, dst_port)])[0][0]


def _acl_struct(acl, keep):
    rules = (_capi.pg_acl_rule * max(1, len(acl["rules"])))()
    for i, r in enumerate(acl["rules"]):
        x = rules[i]
        x.action = r["action"]
        x.has_macip_rule = int(r.get("macip", False))
        x.has_ip_rule = int(r.get("ip_rule", True))
        x.has_ip = int(r.get("ip", True))
        x.has_icmp = int(r.get("icmp", False))
        x.src_network = _b(r.get("src", ""))
        x.dst_network = _b(r.get("dst", ""))
        for name in ("tcp", "udp"):
            sec = r.get(name)
            if sec:
                l4 = getattr(x, name)
                l4.present = 1
                if sec.get("src") is not None:
                    l4.has_src_range = 1
                    l4.src_range.lower_port, l4.src_range.upper_port = sec["src"]
                if sec.get("dst") is not None:
                    l4.has_dst_range = 1
                    l4.dst_range.lower_port, l4.dst_range.upper_port = sec["dst"]
    ing = (C.c_char_p * max(1, len(acl["ingress"])))(*[_b(s) for s in acl["ingress"]])
    eg = (C.c_char_p * max(1, len(acl["egress"])))(*[_b(s) for s in acl["egress"]])
    keep += [rules, ing, eg]
    a = _capi.pg_acl()
    a.name = _b(acl["name"])
    a.rules = C.cast(rules, C.POINTER(_capi.pg_acl_rule))
    a.n_rules = len(acl["rules"])
    a.ingress = C.cast(ing, C.POINTER(C.c_char_p))
    a.n_ingress = len(acl["ingress"])
    a.egress = C.cast(eg, C.POINTER(C.c_char_p))
    a.n_egress = len(acl["egress"])
    return a


class Txn:
    """renderer.Txn (api.go:44-61)."""

    def __init__(self, engine, h):
        self.engine = engine
        self.h = h

    def Render(self, pod, podIP, ingress, egress, removed):
        ns, name = _pod(pod)
        ip = podIP.c() if podIP is not None else None
        ia, ni = _rules_array(ingress)
        ea, ne = _rules_array(egress)
        self.engine._ck(lib.pg_txn_render(self.h, _b(ns), _b(name), C.byref(ip) if ip is not None else None,
                                          ia, ni, ea, ne, int(removed)))
        return self

    def Commit(self):
        h, self.h = self.h, None
        rc = lib.pg_txn_commit(h)
        if rc < 0:
            return PolicyError(rc, lib.pg_last_error(self.engine.h).decode())
        return None

    def __del__(self):
        if getattr(self, "h", None) and lib is not None:
            lib.pg_txn_free(self.h)


class Renderer:
    """The GPU policy renderer (PolicyRendererAPI), EgressOrientation like the ACL renderer."""

    def __init__(self, engine, orientation=EgressOrientation):
        self.engine = engine
        self.h = lib.pg_renderer_new(engine.h, orientation)

    def NewTxn(self, resync):
        return Txn(self.engine, lib.pg_renderer_new_txn(self.h, int(resync)))

    def __del__(self):
        # at interpreter shutdown module globals may already be gone: skip, the process exits
        if getattr(self, "h", None) and lib is not None:
            lib.pg_renderer_free(self.h)
            self.h = None
