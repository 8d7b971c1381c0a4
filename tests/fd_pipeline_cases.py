"""Tables, ANY-protocol placements and oracle answers of the FD group-loop tests (test helper).

Shared by tests/test_fd_group_host.py (pg_debug_classify_host: the kernels' group code on the host,
no GPU) and tests/test_gpu_fd_pipeline.py (the STAGE 4 launches on the device). Nothing here
touches the GPU; everything is built on first use and cached for the process.

Tables: single_matrix's "fd" (302 rules), "empty" and "catch-all", and "split": the smallest
gen-policy-shaped table (workloads.config2's rules, the benchmark's config 2 at more rules) whose
FD walks take their own depths. fastpath.cpp build_fd_blob gives the src and the key walk each its
own trie's depth when they differ by three reads or more, and one common depth otherwise; the
gen-policy table keeps a 5 / 3 shape (common depth 5: 11 reads per lookup) while that fits LDS,
and takes 7 / 4 (12 reads) from 8062 rules on -- found on the CPU by bisection over
pg_debug_walk_stats' reads per lookup, and asserted by test_fd_group_host: an even number of
reads means two different depths (2 d + 1 is odd), 8061 rules still give 11.
"""
import functools

import numpy as np

import single_matrix as sm

SPLIT_RULES = 8062
SM_TABLES = ("fd", "empty", "catch-all")
TABLES = SM_TABLES + ("split",)
# where the ANY-protocol packets (protocol code > 2: the linear scan) sit among a lane's groups of
# four: single_matrix's 2 % at random; exactly tuple j of every group; whole groups (every third
# group, all four tuples); none
PLACEMENTS = ("rand2", "j0", "j1", "j2", "j3", "groups", "none")
ANY_CODES = np.array([3, 7, 255], np.uint8)


def gen_policy_dict_rules(n_rules):
    """the config-2 table at n_rules rules, as the ACL dict rules single_matrix's engines take"""
    from vpp_amd import workloads as W
    w = W.config2(0, n_tuples=16, n_rules=n_rules)
    return w.engine.GetOutboundACL("node1-tap-db0")["rules"]


class SplitTable:
    """single_matrix.Table's fields for the gen-policy table of SPLIT_RULES rules"""

    def __init__(self, n_rules=SPLIT_RULES):
        self.name = "split"
        self.rules = gen_policy_dict_rules(n_rules)
        self.e = sm.engine_with({"t": self.rules}, {})
        self.tid = self.e.table_id("t")
        self.tup = sm.matrix_tuples(self.rules, 21)
        self.n_slots = self.e.num_counter_slots()


@functools.lru_cache(maxsize=None)
def table(name):
    return SplitTable() if name == "split" else sm.table(name)


def reads_per_lookup(t):
    """LDS reads of one FD lookup of table t (pg_debug_walk_stats): src depth + key depth + 1"""
    z = np.zeros(1, np.uint32)
    nl, nm, stage = t.e.debug_walk_stats(t.tid, z, z, np.zeros(1, np.uint16), np.zeros(1, np.uint8))
    assert stage == 4 and nm[0] == 0, (stage, nm)
    return int(nl[0])


def place_any(proto, placement):
    """the table's protocol bytes with the ANY-protocol packets moved to `placement`"""
    n = len(proto)
    if placement == "rand2":
        return proto
    i = np.arange(n)
    plain = np.where(proto > 2, proto % 3, proto).astype(np.uint8)
    if placement == "none":
        return plain
    m = (i // 4) % 3 == 0 if placement == "groups" else (i % 4) == int(placement[1])
    return np.where(m, ANY_CODES[i % len(ANY_CODES)], plain).astype(np.uint8)


class Case:
    """a table's tuples under one placement, with the oracle's verdicts"""

    def __init__(self, name, placement):
        t = table(name)
        self.t, self.e, self.tid, self.n_slots = t, t.e, t.tid, t.n_slots
        src, dst, sport, dport, proto = t.tup
        self.tup = (src, dst, sport, dport, place_any(proto, placement))
        self.act, self.slot = sm.oracle(t.e, t.tid, t.rules, self.tup)
        any_ = self.tup[4] > 2
        g = any_[:len(any_) // 4 * 4].reshape(-1, 4)
        if placement == "none":
            assert not any_.any()
        elif placement == "groups":
            assert (g.all(1) | ~g.any(1)).all() and g.all(1).any() and (~g.any(1)).any()
        elif placement != "rand2":
            j = int(placement[1])
            assert g[:, j].all() and g.sum() == len(g)
        else:
            assert any_.sum() > 1000

    def words(self):
        """the oracle's verdict words (action << 30 | slot), as the kernels write them"""
        return (self.act.astype(np.uint32) << 30) | self.slot.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def case(name, placement):
    return Case(name, placement)
