/*
 * policygpu -- MI355X-native network-policy classification engine for Contiv-VPP.
 *
 * C ABI (the cgo boundary). Every entry point takes plain pointers and sizes; nothing here
 * retains a caller pointer after it returns (cgo pointer-passing rules). All calls are
 * synchronous from the caller's point of view unless a hip stream is passed, and a context
 * is not re-entrant (the reference drives the renderer from one event-loop goroutine,
 * plugins/controller/plugin_controller.go:428).
 *
 * Reference interfaces replaced (file:line under itaimlx/vpp):
 *   renderer.PolicyRendererAPI.NewTxn        plugins/policy/renderer/api.go:33-41
 *   renderer.Txn.Render / Txn.Commit         plugins/policy/renderer/api.go:44-61
 *   renderer.ContivRule                      plugins/policy/renderer/api.go:65-77
 *   acl.Renderer (Init/NewTxn/Commit)        plugins/policy/renderer/acl/acl_renderer.go:93-250
 *   MockACLEngine.ApplyTxn/PutACL/DelACL     mock/aclengine/aclengine_mock.go:151-228, 664-712
 *   MockACLEngine.RegisterPod                mock/aclengine/aclengine_mock.go:144-148
 *   MockACLEngine.Connection*                mock/aclengine/aclengine_mock.go:273-420
 *   MockACLEngine.evalACL / testConnection   mock/aclengine/aclengine_mock.go:424-652 (device)
 *   ipv4net.API getters used by the path     mock/ipv4net/ipv4net_mock.go:70-110
 *   contivconf main/other interfaces         plugins/policy/renderer/acl/acl_renderer.go:70-79
 *   statscollector.RegisterGaugeFunc sink    plugins/statscollector/plugin_impl_statscollector.go:248-261
 *                                            (pg_read_counters is the pull-style value source)
 */
#ifndef POLICYGPU_H
#define POLICYGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (negative errno style) ---------------------------------------- */
#define PG_OK 0
#define PG_ENOENT (-2)    /* unknown pod / ACL / interface                               */
#define PG_EIO (-5)       /* HIP runtime error                                           */
#define PG_ENOMEM (-12)   /* host or device allocation failed                            */
#define PG_EINVAL (-22)   /* invalid argument                                            */
#define PG_EFAULT (-14)   /* the operation failed the way the reference's would (Commit / ApplyTxn error) */

/* ---- enums: values identical to the reference ------------------------------------ */
enum { PG_ACTION_DENY = 0, PG_ACTION_PERMIT = 1 };                 /* renderer.ActionType    */
enum { PG_PROTO_TCP = 0, PG_PROTO_UDP = 1, PG_PROTO_OTHER = 2, PG_PROTO_ANY = 3 }; /* ProtocolType */
enum { PG_ACL_DENY = 0, PG_ACL_PERMIT = 1, PG_ACL_REFLECT = 2, PG_ACL_FAILURE = 3 }; /* ACLAction */
enum { PG_CONN_DENY_SYN = 0, PG_CONN_DENY_SYN_ACK = 1, PG_CONN_ALLOW = 2, PG_CONN_FAILURE = 3 };
enum { PG_ORIENT_INGRESS = 0, PG_ORIENT_EGRESS = 1 };             /* cache.Orientation      */

/* net.IPNet: family 0 = empty network (&net.IPNet{}, "match all"), 4 or 6.
 * addr is the *unmasked* address as the caller holds it (IPv4 in addr[0..3]);
 * prefix_len is the mask's ones (net.CIDRMask(prefix_len, 32|128)).                    */
typedef struct pg_ipnet {
    uint8_t family;
    uint8_t prefix_len;
    uint8_t _pad[2];
    uint8_t addr[16];
} pg_ipnet;

/* renderer.ContivRule */
typedef struct pg_contiv_rule {
    int32_t action;    /* PG_ACTION_*  */
    int32_t protocol;  /* PG_PROTO_*   */
    uint16_t src_port; /* 0 = any      */
    uint16_t dst_port; /* 0 = any      */
    pg_ipnet src;
    pg_ipnet dst;
} pg_contiv_rule;

/* ---- vpp_acl.ACL wire model (vendor/github.com/ligato/vpp-agent/api/models/vpp/acl/acl.proto:24-113)
 * Strings are CIDRs as rendered by the reference ("" = field unset).                   */
typedef struct pg_port_range {
    uint32_t lower_port;
    uint32_t upper_port;
} pg_port_range;

typedef struct pg_l4 {
    uint8_t present;       /* section exists (ipRule.Tcp / ipRule.Udp != nil) */
    uint8_t has_src_range; /* SourcePortRange != nil                          */
    uint8_t has_dst_range; /* DestinationPortRange != nil                     */
    uint8_t _pad;
    pg_port_range src_range;
    pg_port_range dst_range;
} pg_l4;

typedef struct pg_acl_rule {
    int32_t action; /* vpp_acl.ACL_Rule_Action: 0 DENY, 1 PERMIT, 2 REFLECT */
    uint8_t has_macip_rule;
    uint8_t has_ip_rule;
    uint8_t has_ip;
    uint8_t has_icmp;
    const char* src_network;
    const char* dst_network;
    pg_l4 tcp;
    pg_l4 udp;
} pg_acl_rule;

typedef struct pg_acl {
    const char* name;
    const pg_acl_rule* rules;
    size_t n_rules;
    const char* const* ingress; /* Interfaces.Ingress */
    size_t n_ingress;
    const char* const* egress;  /* Interfaces.Egress  */
    size_t n_egress;
} pg_acl;

typedef struct pg_acl_op {
    const char* key;     /* "config/vpp/acls/v2/acl/<name>" (vpp_acl.Key) */
    const pg_acl* value; /* NULL = delete                                  */
} pg_acl_op;

/* ---- tuples (device pointers, SoA) ------------------------------------------------- */
typedef struct pg_tuple_soa {
    const uint32_t* src_ip;   /* host-order IPv4                      */
    const uint32_t* dst_ip;
    const uint16_t* src_port; /* only read by PG_MODE_CONN            */
    const uint16_t* dst_port;
    const uint8_t* proto;     /* PG_PROTO_*                           */
} pg_tuple_soa;

/* Classification modes.
 *  SINGLE: evalACL(table, src, dst, proto, dport) for one table         (configs 1,2,4)
 *  PERPOD: evalACL(outbound ACL of the interface the packet leaves by --
 *          dst pod's TAP or the node-output interface)                  (config 3)
 *  CONN:   testConnection over the src/dst interfaces resolved by IP    (config 5)
 * Output word: bits 31-30 = ACLAction (SINGLE/PERPOD) or ConnAction (CONN),
 *              bits 29-0  = counter slot of the deciding rule (see pg_num_counter_slots). */
enum { PG_MODE_SINGLE = 0, PG_MODE_PERPOD = 1, PG_MODE_CONN = 2 };
#define PG_VERDICT_ACTION(w) ((uint32_t)(w) >> 30)
#define PG_VERDICT_SLOT(w) ((uint32_t)(w)&0x3FFFFFFFu)

/* ---- engine context (one GPU) ------------------------------------------------------ */
typedef struct pg_ctx pg_ctx;
typedef struct pg_renderer pg_renderer;
typedef struct pg_txn pg_txn;

/* One context per GPU. Every call that touches the device makes hip_device current for its
 * duration and restores the caller's current device afterwards, so contexts on different GPUs
 * can be driven from one process, and a cgo caller may call from any OS thread. A context is
 * not re-entrant; distinct contexts may be used concurrently from different threads. */
pg_ctx* pg_create(int hip_device);
int pg_ctx_device(const pg_ctx* ctx);
/* Tuning knobs (key, value):
 * launches -- "blocks_per_cu" (cap on resident workgroups per CU of the classify grid;
 * default 0 = as many as registers/LDS allow), "stage_max_words" (largest table blob staged
 * in LDS, default 16384 = 64 KiB), "stage_root_max_words" (larger blobs: header + src-trie
 * root staged, default 16400), "node_path" (1/0: classify PERPOD / CONN through the node
 * classifier when it exists, default 1; 0 = per-table blobs and the IP hash),
 * "node_stage_max_words" (largest node image staged in LDS, default 16384),
 * "node_common_lds_max" (LDS bytes up to which the node image's common-row section is staged,
 * default 80 KiB), "block_stage" (workgroup size of LDS-staged classify launches: 256, 512 or
 * 1024; default 0 = per mode), "hist_window" (hit counters of a table set with more than 16382
 * slots: LDS cells kept for the classified table's first rules -- its default-deny slot and last
 * rule always get one -- the rest counted with global atomics; default 4096), "node_hist_cells"
 * (PERPOD / CONN launches over a table set with more than 16382 slots: cells of the LDS cache the
 * hit counters go through -- the hottest slots of each workgroup's stream claim them, the rest
 * take global atomics -- rounded down to a power of two, up to 8192; default 256, < 16 = none);
 * table compiler (the context recompiles and re-uploads on its next use; hit counters carry over)
 * -- "root_bits_max" (cap of the src/key trie root stride, 4..16, default 16), "node_build"
 * (1/0: build the node classifier for PERPOD / CONN, default 1), "node_root_bits" (its IPv4 /
 * key trie root stride cap, default 12), "node_key_root_bits" (cap of the uniform layout's
 * key trie root stride, 2..10; the strides tried are 2, 6 and 10 (18 - root a multiple of 4),
 * so the cap is rounded down to one of them -- 10 saves a level for ~4 KiB of image; default
 * 6), "lc_lds" (table blobs of at least this many words are
 * rebuilt with level-compressed 12/16-bit trie strides and keep them when the result still
 * fits in LDS; default 4096, 0 = off; blobs too large for LDS are always level-compressed),
 * "lc_dense12" (boundaries a subtree needs for a 12-bit stride, default 16), "lc_max_stride"
 * (widest level-compressed stride: 12, 16 or 18, default 16), "lc_root_bits" (src-trie root
 * stride cap of blobs read from HBM, whose root alone a launch stages in LDS: 4..14, default
 * 13), "candi" (1/0: candidates inline in the 8-B trie entries of HBM-resident candidate tables
 * no live rule of which tests dst, default 1), "candi_window_bits" (such a table's LDS window:
 * the terminal entries of the 2^bits addresses of the aligned window where its earliest rules
 * sit, staged with the root, so a lookup there makes no trie gather; 0..13, 0 = none, default
 * 11; left out when it would not stage with the root), "candi_window_root_bits" (root stride cap
 * of a table with a window, default 12: root + window in 32 KiB), "fd" (1/0: fixed-depth form of dst-independent
 * cross-product tables, default 1), "node_common" (1/0: common-row section of node
 * images, default 1), "node_uniform" (1/0: the node's uniform cross layout where every table
 * is covered and none is in PAIR form, default 1), "node_list_table" (1/0: in the uniform layout
 * a node cross entry whose table still has dst-specific rules ahead of its verdict resolves them
 * by one read of a list-verdict table indexed by the dst's node IP class -- the IPv4 classes then
 * also separate those rules' dst prefixes -- instead of walking dst records; 0 = records, which
 * rules the uniform layout out for a set with such rules; default 1), "node_list_words"
 * (record form: node dst records up to this many words go into the node image, so a launch that
 * stages the image walks them in LDS; default 4096, 0 = never), "pair" (1/0: the PAIR structure -- src x dst classes, then x key classes
 * -- for tables the cross product cannot take, default 1; 0 = candidate lists; 2 = wherever it
 * fits, for tests), "launch_max_tuples" (a pg_classify batch larger than this takes several
 * kernel launches of at most this many tuples, in order on the stream; a multiple of 64, 0 =
 * the largest a launch's 32-bit stream offsets allow, 2^30 - 64; default 0; pg_reach_observed
 * cuts its flow batch by the same knob), "classes_hash_bits"
 * (pg_reach_classes keeps only this many low bits of every signature, 0..64, 0 = every signature
 * equal; the result does not depend on it, only the rounds of the equality check do -- for tests
 * that reach those rounds at small shapes; default 64), "rules_hist_cells" (pg_reach_rules: cap of
 * the u32 LDS cells a workgroup counts into before its global atomics, both histograms together,
 * 0..16384; what does not fit is counted with global atomics, 0 = global atomics only; the result
 * does not depend on it -- for tests that reach the global path at small shapes; default 16384 =
 * whatever fits), "rules_wave_agg" (pg_reach_rules: 1/0, the lanes of a wave that hit the first
 * active lane's cell add with one atomic instead of one each; the result does not depend on it;
 * default 1, DESIGN.md has the measurement), "observed_lds_bytes" (pg_reach_observed: cap of the
 * LDS bytes its two address tables may take in a workgroup, 0..163840; a table that does not fit
 * is probed in HBM, 0 = never staged; the result does not depend on it -- for tests that reach the
 * HBM probes at small shapes; default 163840 = whatever fits), "observed_test_first"
 * (pg_reach_observed: a cell's word is loaded before its atomic OR and the atomic skipped where the
 * bit shows; 0 = always the atomic, 1 = a plain load, 2 = a load that the CU's L1 does not answer;
 * the result does not depend on it; default 1, DESIGN.md has the measurement), "cost_lds_bytes"
 * (pg_reach_cost: cap of the LDS bytes a workgroup may take for its cost row and the weights beside
 * its two bit vectors, 0..163840; the weights are dropped from LDS first and read through L2, then
 * the row, which then lives in global memory under global atomics, 0 = nothing staged; the result
 * does not depend on it -- for tests that reach all three variants at small shapes; default 163840 =
 * whatever fits).
 * pg_ctx_set_tuning sets one context's knob; pg_set_tuning sets the process default that
 * contexts created afterwards start from. PG_EINVAL for an unknown key or a value out of range. */
int pg_ctx_set_tuning(pg_ctx* ctx, const char* key, int value);
int pg_ctx_get_tuning(const pg_ctx* ctx, const char* key, int* value); /* ctx NULL: process default */
int pg_set_tuning(const char* key, int value);
void pg_destroy(pg_ctx* ctx);
const char* pg_last_error(const pg_ctx* ctx);
const char* pg_version(void);

/* ipv4net / contivconf roles the renderer and the engine depend on */
int pg_set_pod_if_name(pg_ctx* ctx, const char* pod_namespace, const char* pod_name, const char* if_name);
int pg_set_host_interconnect_if_name(pg_ctx* ctx, const char* if_name);
int pg_set_main_interface_name(pg_ctx* ctx, const char* if_name);
int pg_set_other_vpp_interfaces(pg_ctx* ctx, const char* const* if_names, size_t n);
int pg_set_vxlan_bvi_if_name(pg_ctx* ctx, const char* if_name);
/* MockACLEngine.RegisterPod. pg_classify's PERPOD / CONN modes and the reachability audits resolve
 * an IPv4 address to the pod registered with it. Of several pods registered with one address the
 * last in PodID order (namespace, then name; not the order of the calls) answers for it, whatever
 * its kind: a pod of another node takes a local pod's address over and the other way round, a
 * local pod without an interface makes it unresolvable. (The reference keeps pods by ID and has no
 * such rule; pg_connections, which takes pod IDs, is not affected.) */
int pg_register_pod(pg_ctx* ctx, const char* pod_namespace, const char* pod_name, const char* ip, int another_node);

/* ---- renderer (PolicyRendererAPI) -------------------------------------------------- */
pg_renderer* pg_renderer_new(pg_ctx* ctx, int orientation);
void pg_renderer_free(pg_renderer* r);
pg_txn* pg_renderer_new_txn(pg_renderer* r, int resync);
int pg_txn_render(pg_txn* txn, const char* pod_namespace, const char* pod_name, const pg_ipnet* pod_ip,
                  const pg_contiv_rule* ingress, size_t n_ingress, const pg_contiv_rule* egress, size_t n_egress,
                  int removed);
int pg_txn_commit(pg_txn* txn); /* renders, applies to the engine, frees txn */
void pg_txn_free(pg_txn* txn);  /* abandon without commit                    */

/* ---- ACL ingestion (vpp-agent key space) and introspection -------------------------- */
int pg_apply_txn(pg_ctx* ctx, int resync, const pg_acl_op* ops, size_t n_ops);
int pg_num_acls(pg_ctx* ctx);
int pg_num_acl_changes(pg_ctx* ctx);
int pg_num_committed_txns(pg_ctx* ctx);
/* JSON of one ACL ({"name","ingress","egress","rules":[...]}) -> bytes needed (incl. NUL). */
int pg_acl_json(pg_ctx* ctx, const char* acl_name, char* buf, size_t cap);
/* JSON array of all installed ACL names (sorted) -> bytes needed (incl. NUL) */
int pg_acl_names_json(pg_ctx* ctx, char* buf, size_t cap);
/* names of the ACLs bound to an interface ("" when none) */
int pg_interface_acls(pg_ctx* ctx, const char* if_name, char* inbound, size_t in_cap, char* outbound,
                      size_t out_cap);

/* ---- device tables and classification ---------------------------------------------- */
int pg_sync_tables(pg_ctx* ctx); /* compile + upload (double-buffered swap); implicit in classify */
int pg_table_id(pg_ctx* ctx, const char* acl_name);
int pg_num_tables(pg_ctx* ctx);
int pg_num_counter_slots(pg_ctx* ctx);
/* global rule slot -> (table id, rule index in its ACL); rule index -1 for a table's
 * default-deny slot; table id -1 for the "no ACL" (permit) slot */
int pg_slot_info(pg_ctx* ctx, uint32_t slot, int32_t* table_id, int32_t* rule_index);
/* table -> (first rule slot, rules, default-deny slot) */
int pg_table_info(pg_ctx* ctx, int table_id, uint32_t* rule_base, uint32_t* n_rules, uint32_t* default_slot);

/* classification structure of a table: flags (1 cross, 2 dst lists, 4 candidate mode,
 * 8 linear fallback), blob bytes, src / key equivalence classes */
int pg_table_stats(pg_ctx* ctx, int table_id, uint32_t* flags, uint32_t* blob_bytes, uint32_t* n_src_classes,
                   uint32_t* n_key_classes);

int pg_classify(pg_ctx* ctx, int mode, int table_id, const pg_tuple_soa* tuples, uint64_t n, uint32_t* out,
                uint64_t* counters, void* hip_stream);

/* TESTS ONLY -- never on the classify path: walk one ACL's compiled classification blob on
 * the host (the same walk code the kernels instantiate) for n host tuples, so the table
 * compiler can be checked against the oracle without a GPU. Does not touch the device. */
int pg_debug_walk_blob(pg_ctx* ctx, const char* acl_name, const uint32_t* src, const uint32_t* dst,
                       const uint16_t* dst_port, const uint8_t* proto, uint64_t n, uint32_t* out);
/* TESTS ONLY -- never on the classify path: pg_classify's per-tuple code (classify.hpp, the
 * same templates the kernels instantiate) run on the host over host tuples, any mode, with
 * optional host u64 counters. flags: bit 0 = node classifier when it exists (else the
 * per-table path), bit 1 = the predicated trie walks the kernels use on LDS-staged images
 * (else the branching ones they use on HBM-resident ones), bit 2 = the node image's
 * common-row section when it was built (the kernels use it when it fits their LDS budget).
 * Does not touch the device. */
int pg_debug_classify_host(pg_ctx* ctx, int mode, int table_id, const pg_tuple_soa* tuples, uint64_t n,
                           uint32_t* out, uint64_t* counters, int flags);
/* TESTS ONLY, the same for the reachability matrix: pg_debug_reach_matrix_host, declared with
 * pg_reach_matrix below. */
/* TESTS ONLY -- never on the classify path: where the end-point table (the open-addressing hash
 * over the registered pods' IPv4 addresses that the per-table path, the node kernels' ANY-protocol
 * pass and form B of the reachability audits resolve an address with) finds each of n addresses,
 * read off the compiled host image by a plain loop: out_slot[i] = the cell the probe of ips[i]
 * starts at, out_steps[i] = the 16-byte cells it reads until it hits the address or an empty cell
 * (1 = the first cell decides), *out_cap = the table's cells (a power of two; a probe wraps from
 * cell cap - 1 to cell 0). Any output may be null. Tests use it to show that their addresses reach
 * a collision chain, a wrap or a long miss -- never for an expected verdict. Does not touch the
 * device. */
int pg_debug_endpoint_probe(pg_ctx* ctx, const uint32_t* ips, uint64_t n, uint32_t* out_steps, uint32_t* out_slot,
                            uint32_t* out_cap);
/* TESTS ONLY -- never on the classify path: install n host counters (e.g. from
 * pg_debug_classify_host) as the LOCAL or CLUSTER snapshot in the currently compiled slot layout,
 * so the snapshot readers below can be tested without a GPU. n must equal the slot count. */
int pg_debug_set_snapshot(pg_ctx* ctx, int which, const uint64_t* counters, size_t n);
/* TESTS ONLY -- never on the classify path: the per-stream launch-mark bookkeeping of PERPOD / CONN launches
 * (device.hpp StreamSlots, which pg_classify uses to hand a launch's deferred ANY-protocol packets
 * to the k_node_any launched after it on the same stream) replayed for n launches on the given
 * stream handles: slot_out[k] = the mark word launch k writes, seq_out[k] = its launch number. No
 * device work. */
int pg_debug_stream_slots(const uint64_t* streams, size_t n, uint32_t* slot_out, uint32_t* seq_out);
/* TESTS / MEASUREMENT ONLY -- never on the classify path: per tuple, the loads a SINGLE-mode
 * launch on table_id makes of the table's classification structure, split by where the launch
 * finds the word: lds_reads (the LDS-staged part) and mem_reads (HBM / L2 gathers; rule reads of
 * the linear scan for ANY-protocol packets). *stage = the staging the launch uses (device.hip
 * k_classify STAGE: 0 none, 1 blob, 2 src root, 4 FD blob, 5 FD prefix). Runs the kernels' walk
 * code on the host with counting loaders; does not touch the device. */
int pg_debug_walk_stats(pg_ctx* ctx, int table_id, const pg_tuple_soa* tuples, uint64_t n, uint32_t* lds_reads,
                        uint32_t* mem_reads, int* stage);
/* TESTS ONLY -- never on the classify path: the launch a SINGLE-mode pg_classify on table_id makes
 * under the context's launch knobs, with hit counters (counters != 0) or without, from the one
 * function the launch itself dispatches on (device.hpp single_launch_plan). *stage_code = the
 * full k_classify STAGE: 4 FD blob in LDS, 5 FD prefix in LDS; 1 blob in LDS, 2 src root in LDS,
 * 0 nothing staged (linear-flagged tables too); and for tables no rule of which tests dst (the dst
 * stream is not read) 9, 10, 8 likewise and 14 = a CANDI table's root and window in LDS.
 * *stage_words = blob words staged; *hist_cells = cells of the LDS hit-counter histogram without
 * its two extra cells (every slot, or the "hist_window" window; 0 without counters). Any output
 * may be null. Does not touch the device. */
int pg_debug_launch_plan(pg_ctx* ctx, int table_id, int counters, int* stage_code, uint32_t* stage_words,
                         uint32_t* hist_cells);
/* TESTS ONLY: the geometry of the last classify kernel the calling thread launched (pg_classify):
 * *block = threads per workgroup, *grid = workgroups launched, *resident = the workgroups the
 * device holds at once under the launch knobs (the most a grid takes; a launch of more groups
 * than resident * block strides over them). Zeros before the thread's first launch. */
int pg_debug_last_launch(int* block, int* grid, int* resident);
/* TESTS ONLY -- never on the classify path: the launch a PERPOD / CONN pg_classify makes of the
 * compiled table set under the context's launch knobs, with hit counters (counters != 0) or
 * without, from the one function the launch itself dispatches on (device.hpp node_launch_plan).
 *   path            1 = the node classifier, 0 = the per-table path ("node_path" 0, or no node)
 *   stage_code      the full k_classify STAGE of the node kernel: 3 = the node image with its
 *                   common-row section staged in LDS, 1 = the base image staged, 0 = the image
 *                   read from HBM; + 32 node sets without PAIR tables, + 96 the uniform layout,
 *                   + 96 + 128 with wide records; + 16 counters in an LDS histogram of every
 *                   slot, + 16 + 256 in 16-bit cells. Per-table path: 0
 *   stage_words     image words staged
 *   records_staged  1 = the dst records are read from the image (staged with it, or with
 *                   stage_code 0 from HBM), 0 = from the cross array (or there are none)
 *   hist_kind       PG_HIST_*: no counters; every slot in 32-bit LDS cells; every slot in 16-bit
 *                   LDS cells; the node's LDS slot cache ("node_hist_cells", sets of more than
 *                   16382 slots); global atomics only; the first "hist_window" slots in LDS (the
 *                   per-table path over such a set)
 *   hist_cells      LDS cells without the scheme's extra cells; hist_bytes: its LDS bytes
 *   defers_any      1 = a k_node_any launch follows for the ANY-protocol packets
 * mode: PG_MODE_PERPOD or PG_MODE_CONN. Does not touch the device. */
enum { PG_HIST_NONE = 0, PG_HIST_FULL32 = 1, PG_HIST_HALF16 = 2, PG_HIST_CACHE = 3, PG_HIST_GLOBAL = 4,
       PG_HIST_WINDOW = 5 };
typedef struct pg_node_launch_plan {
    int path, stage_code;
    uint32_t stage_words;
    int records_staged, hist_kind;
    uint32_t hist_cells, hist_bytes;
    int defers_any;
} pg_node_launch_plan;
int pg_debug_node_launch_plan(pg_ctx* ctx, int mode, int counters, pg_node_launch_plan* plan);
/* node classifier (PERPOD / CONN) size: IPv4 classes, L4-key classes, LDS image bytes,
 * cross-table bytes; PG_ENOENT when it was not built */
int pg_node_stats(pg_ctx* ctx, uint32_t* ip_classes, uint32_t* key_classes, uint64_t* image_bytes,
                  uint64_t* cross_bytes);
/* node image layout: bytes of the base image (without the common-row section), and how many of
 * the covered (table, IPv4 class) pairs read the table's common row from the image instead of
 * the cross table (0 when the section was not built); PG_ENOENT when there is no node */
int pg_node_common_stats(pg_ctx* ctx, uint64_t* base_image_bytes, uint64_t* common_pairs, uint64_t* pairs);
/* the node classifier's dst records (the dst-specific rules its cross entries still test, record
 * form): their bytes, and whether a copy ends the node image (tuning "node_list_words"); 0 bytes in
 * the list-table form (pg_node_list_table_stats); PG_ENOENT: no node */
int pg_node_list_stats(pg_ctx* ctx, uint64_t* record_bytes, int* in_image);
/* the node classifier's list-verdict table (tuning "node_list_table"): its bytes in the cross
 * array (0 = the record form, or no lists); PG_ENOENT: no node */
int pg_node_list_table_stats(pg_ctx* ctx, uint64_t* table_bytes);
/* 1 when the node classifier uses the uniform cross layout (every table covered, none in PAIR
 * form, tuning "node_uniform": entry addresses computed, no per-table info reads), 2 when it does
 * with wide class records (255 tables or more: 16-bit table ids, 32-bit common-row marks), else
 * 0; PG_ENOENT: no node */
int pg_node_uniform(pg_ctx* ctx);
/* reference-shaped linear-scan kernel (K1) on one table, for validation and comparison */
int pg_classify_linear(pg_ctx* ctx, int table_id, const pg_tuple_soa* tuples, uint64_t n, uint32_t* out,
                       void* hip_stream);
/* MEASUREMENT -- not part of the reference's interface: the stream ceiling of a pg_classify
 * launch. Issues exactly the loads a launch makes of the tuple fields (src, dst_port, proto;
 * dst_ip when fields & 1, src_port when fields & 2) and its 4-B store per tuple, with the same
 * vector widths and grid, but no classification (out[i] = xor of the fields). bench.py times
 * it beside the classify kernel: classify rate / probe rate = how close the classification
 * comes to what moving its own bytes costs on this GPU. Fields and out must be vector-aligned
 * (16-B src / dst / out); PG_EIO otherwise. */
int pg_stream_probe(pg_ctx* ctx, int fields, const pg_tuple_soa* tuples, uint64_t n, uint32_t* out,
                    void* hip_stream);
/* device-resident per-rule hit counters (u64, pg_num_counter_slots entries) */
uint64_t* pg_counters_device(pg_ctx* ctx);
int pg_reset_counters(pg_ctx* ctx, void* hip_stream);
/* waits for this context's classify launches, copies min(n, slots) counters -> slots copied
 * (also refreshes the LOCAL host snapshot) */
int pg_read_counters(pg_ctx* ctx, uint64_t* host_out, size_t n);
/* ---- host snapshots: the statscollector value source -----------------------------------
 * (RegisterGaugeFunc, plugin_impl_statscollector.go:248-261: a pull-style gauge whose value
 * function runs at scrape time, on its own goroutine.) The library keeps two host copies of the
 * counters, each with the slot layout it was counted in; reading them never touches the GPU and
 * is safe from any thread while the context classifies:
 *   PG_SNAP_LOCAL    this GPU's counts, as of the last pg_read_counters
 *   PG_SNAP_CLUSTER  the sum over the communicator, as of the last pg_allreduce_counters*
 *   PG_SNAP_GAUGE    CLUSTER once the context has a communicator, else LOCAL: a monotonic
 *                    source either way (neither call writes the other's copy)
 * Slots are renumbered whenever the tables are recompiled, so a gauge should be keyed by a
 * stable rule identity -- (ACL name, rule index) -- and read with pg_counter_of_rule, which
 * resolves it in the snapshot's own layout. Counts survive a recompile: every ACL present before
 * and after it under the same name with the same rules keeps its counts (its rules and its
 * default deny), as do "no ACL" and "unresolved" -- in the device counters (carried to the new
 * slots when the new tables are uploaded) and in both host snapshots (when they are compiled);
 * the slots of new or changed ACLs start at zero. */
enum { PG_SNAP_GAUGE = 0, PG_SNAP_LOCAL = 1, PG_SNAP_CLUSTER = 2 };
/* PG_SNAP_GAUGE snapshot: copies min(n, slots) -> number of slots in it (0 before the first read) */
int pg_counters_snapshot(const pg_ctx* ctx, uint64_t* host_out, size_t n);
/* slots [first, first + n) of a snapshot (clipped to its size) -> number copied; *layout_gen
 * (optional) = the layout generation of that snapshot (0: none taken yet) */
int pg_counters_snapshot_range(const pg_ctx* ctx, int which, uint32_t first, uint32_t n, uint64_t* host_out,
                               uint64_t* layout_gen);
/* one rule's count in a snapshot by its stable identity: ACL name and rule index (-1: the ACL's
 * default deny); acl_name NULL with rule_index -1 = the "no ACL" slot, -2 = the unresolved-
 * interface slot. O(log ACLs), no allocation. PG_ENOENT: no snapshot yet, or the ACL / index
 * does not exist in the snapshot's layout. *layout_gen (optional) as above. */
int pg_counter_of_rule(const pg_ctx* ctx, int which, const char* acl_name, int rule_index, uint64_t* value,
                       uint64_t* layout_gen);
/* generation of the compiled slot layout (increments on every recompile; 0 = never compiled):
 * an agent re-registers gauges for new (ACL, rule) identities when it changes. Any thread. */
uint64_t pg_counter_layout_gen(const pg_ctx* ctx);

/* ---- RCCL over xGMI: per-rule hit counters summed over the GPUs of a node -------------
 * (the statscollector path). The classify path itself has no exchange.
 * Multi-process (one process per GPU): rank 0 calls pg_comm_unique_id and hands the bytes to
 * the other ranks (any side channel), every rank calls pg_comm_init_rank on its context.
 * One process driving several GPUs: pg_comm_init_all over one context per GPU.
 * pg_allreduce_counters / pg_allreduce_counters_all first check that every rank compiled the
 * same counter layout (slots, ACL names, rules per ACL; PG_EFAULT if not, nothing reduced), then
 * sum a device copy of the counters (ncclAllReduce u64 sum) into the host snapshots. The
 * device counters keep this rank's own counts (pg_read_counters still returns them), so a
 * periodic gauge may all-reduce again without a reset in between. The caller's current device
 * is restored on every return path.
 * Synchronous. RCCL (librccl.so.1) is loaded on first use. */
#define PG_COMM_ID_BYTES 128
int pg_comm_unique_id(uint8_t id[PG_COMM_ID_BYTES]);
int pg_comm_init_rank(pg_ctx* ctx, int nranks, const uint8_t id[PG_COMM_ID_BYTES], int rank);
int pg_comm_init_all(pg_ctx* const* ctxs, int n);
int pg_comm_destroy(pg_ctx* ctx);
int pg_comm_rank(const pg_ctx* ctx, int* rank, int* nranks); /* PG_ENOENT: no communicator */
int pg_allreduce_counters(pg_ctx* ctx, void* hip_stream);
int pg_allreduce_counters_all(pg_ctx* const* ctxs, int n);

/* ---- synthetic input generation on device (bench / parity workloads) ----------------- */
typedef struct pg_gen_spec {
    uint64_t seed;
    uint64_t index_base;      /* global index of tuple 0 (multi-GPU shards)               */
    int32_t table_id;         /* >= 0: "inside a rule" sampling from this table           */
    uint32_t inside_pct;      /* % of tuples sampled inside a rule's predicate            */
    const uint32_t* ip_pool;  /* host array: pool of "known" IPs (pods / internet hosts)  */
    uint32_t n_ip_pool;
    uint32_t pool_pct;        /* % of src/dst drawn from ip_pool (else uniform u32)       */
    const uint16_t* port_pool;/* host array of popular dst ports                          */
    uint32_t n_port_pool;
    uint32_t port_pool_pct;   /* % of dst ports drawn from port_pool                      */
    uint32_t tcp_pct, udp_pct;/* protocol mix (rest OTHER)                                */
    const uint32_t* zipf_cdf; /* host array, n_rules+1 entries scaled to 2^32: rule index  *
                               * follows it (config 4); NULL = uniform rule choice        */
    uint32_t nomatch_pct;     /* % forced outside every rule's src (config 4)             */
    uint32_t dst_pool_pct;    /* % of dst drawn from ip_pool (config 3/5: local pods)     */
} pg_gen_spec;

int pg_gen_tuples(pg_ctx* ctx, const pg_gen_spec* spec, uint64_t n, uint32_t* src_ip, uint32_t* dst_ip,
                  uint16_t* src_port, uint16_t* dst_port, uint8_t* proto, void* hip_stream);

/* ---- Connection* (MockACLEngine) evaluated on the device ------------------------------ */
typedef struct pg_conn_query {
    int32_t kind;              /* 0 PodToPod, 1 PodToInternet, 2 InternetToPod */
    const char* src_namespace; /* pod endpoints                                  */
    const char* src_name;
    const char* dst_namespace;
    const char* dst_name;
    const char* src_ip;        /* internet endpoints (string, net.ParseIP)       */
    const char* dst_ip;
    int32_t protocol;
    uint16_t src_port;
    uint16_t dst_port;
} pg_conn_query;
/* out[i] = ConnAction; out_slot (optional) = deciding slot per query */
int pg_connections(pg_ctx* ctx, const pg_conn_query* q, size_t n, int32_t* out, uint32_t* out_slot);

/* ---- reachability matrix: testConnection over src x dst x service on the device -------
 * "Which end points can reach which, on which services?" after a policy commit. Pair (service
 * v, src i, dst j) gets exactly the verdict word pg_classify(PG_MODE_CONN) gives the tuple
 * (src_ip[i], dst_ip[j], services[v].src_port, services[v].dst_port, services[v].protocol): end
 * points are resolved from the addresses (a pod of this node, a remote pod, a non-pod address),
 * with the same preamble FAILUREs and "unresolved" slot; the deciding slot is the slot of the
 * last evaluation. What depends on one end point or one service alone (trie walks, iphash
 * probes) is computed once per end point / service, not once per pair.
 *   out_packed  device, n_svc * n_src * pg_reach_row_words(n_dst) words: the ConnAction of (v, i,
 *               j) in bits [2 * (j & 15), 2 * (j & 15) + 1] of word (v * n_src + i) * row_words +
 *               (j >> 4); the padding bits of a row's last word are zero
 *   out_words   device, optional: n_svc * n_src * n_dst full verdict words, row-major (drill-down
 *               to the deciding rule with pg_slot_info)
 * The call is an audit, not traffic: it never touches the hit counters or their snapshots.
 * Like pg_gen_tuples it compiles and uploads stale tables first, copies the small host arrays
 * in, enqueues its kernels in order on hip_stream and may synchronise that stream before it
 * returns. A zero n_src, n_dst or n_svc: PG_OK, nothing written. PG_EINVAL: null spec or
 * out_packed, a side longer than 2^20, more than 4096 services. IPv4 only. */
typedef struct pg_service {
    int32_t protocol;         /* PG_PROTO_*; codes > 3 behave as in pg_classify (ANY) */
    uint16_t src_port, dst_port;
} pg_service;
typedef struct pg_reach_spec {
    const uint32_t* src_ip;   /* host arrays, host-order IPv4; duplicates allowed */
    size_t n_src;
    const uint32_t* dst_ip;
    size_t n_dst;
    const pg_service* services;
    size_t n_svc;
} pg_reach_spec;
size_t pg_reach_row_words(size_t n_dst); /* (n_dst + 15) / 16 */
int pg_reach_matrix(pg_ctx* ctx, const pg_reach_spec* spec, uint32_t* out_packed, uint32_t* out_words,
                    void* hip_stream);
/* TESTS ONLY -- never on the audit path: pg_reach_matrix's per-end-point, per-service and
 * per-pair code (reach.hpp, the same templates the kernels instantiate) run on the host with
 * host output arrays. flags: bit 0 = the node classifier when it exists and is uniform (else the
 * per-table path), as in pg_debug_classify_host. Does not touch the device. */
int pg_debug_reach_matrix_host(pg_ctx* ctx, const pg_reach_spec* spec, uint32_t* out_packed, uint32_t* out_words,
                               int flags);

/* ---- port sweep: the open dst ports of every src x dst pair on the device ----------------
 * "Between these end points, which ports are open?" For a fixed protocol (TCP or UDP) and src
 * port, evalACL tests a packet's dst port only against the rules' dst-port ranges, so the verdict
 * of (src, dst, protocol, src_port, dst_port) is constant inside every elementary interval that
 * the rules' dst-port bounds cut 0..65535 into. A sweep over all 65,536 ports is K evaluations
 * per pair -- tens to hundreds on a real table set.
 *
 * pg_port_intervals: the elementary dst-port intervals of a protocol (PG_PROTO_TCP or
 * PG_PROTO_UDP) over every installed ACL: lo[0] = 0 < lo[1] < ... ascending; interval k =
 * [lo[k], lo[k+1] - 1], the last ends at 65535. Returns K (>= 1; 1 without ACLs), copies
 * min(K, cap) bounds (lo may be null when cap is 0). Two ports of one interval get the same
 * (action, rule index) from evalACL in every installed ACL, for every src / dst. Every lo[k], k >
 * 0, is lower & 0xFFFF or (upper & 0xFFFF) + 1 of the dst range of some installed rule's L4
 * section of that protocol -- the bounds as evalACL compares them, after its uint16 truncation --
 * so K <= 2 * rules + 1; rules that can never match still cut. Host only, no device work.
 * PG_EINVAL: another protocol. */
int pg_port_intervals(pg_ctx* ctx, int protocol, uint32_t* lo, size_t cap);
/* pg_reach_ports: with K and lo[] of pg_port_intervals(protocol) and row_words =
 * pg_reach_row_words(K),
 *   out_codes  device, required, n_src * n_dst * row_words words: the ConnAction of pair (i, j) on
 *              interval k in bits [2 * (k & 15), 2 * (k & 15) + 1] of word (i * n_dst + j) *
 *              row_words + (k >> 4); the padding bits of a pair's last word are zero
 *   out_open   device, optional, n_src * n_dst words: per pair the number of dst ports whose
 *              ConnAction is PG_CONN_ALLOW (the lengths of its ALLOW intervals), 0..65536
 *   out_words  device, optional, n_src * n_dst * K words: the full verdict word of every (pair,
 *              interval), bit-identical to pg_classify(PG_MODE_CONN) on (src_ip[i], dst_ip[j],
 *              src_port, lo[k], protocol)
 * End-point resolution, preamble FAILUREs, the "unresolved" slot and the slot reported (that of
 * the last evaluation) are pg_reach_matrix's. The call never touches the hit counters or their
 * snapshots. Like pg_reach_matrix it compiles and uploads stale tables first, enqueues in order
 * on hip_stream and may synchronise it. An empty side: PG_OK, nothing written. PG_EINVAL: a null
 * spec or out_codes; a protocol other than TCP / UDP; a side longer than 2^20; n_src * n_dst *
 * row_words >= 2^32; n_intervals different from the partition's current K (the ACLs changed
 * since pg_port_intervals; pg_last_error says so). */
typedef struct pg_port_sweep_spec {
    const uint32_t* src_ip;   /* host arrays, host-order IPv4; duplicates allowed */
    size_t n_src;
    const uint32_t* dst_ip;
    size_t n_dst;
    int32_t protocol;         /* PG_PROTO_TCP | PG_PROTO_UDP */
    uint16_t src_port;        /* fixed: the SYN-ACK key */
    uint16_t _pad;
    size_t n_intervals;       /* K the caller sized its buffers for */
} pg_port_sweep_spec;
int pg_reach_ports(pg_ctx* ctx, const pg_port_sweep_spec* spec, uint32_t* out_codes, uint32_t* out_open,
                   uint32_t* out_words, void* hip_stream);
/* TESTS ONLY -- never on the audit path: pg_reach_ports's per-pair code (ports.hpp, the same
 * templates the kernel instantiates) on the host with host output arrays. flags: bit 0 as in
 * pg_debug_reach_matrix_host. Does not touch the device. */
int pg_debug_reach_ports_host(pg_ctx* ctx, const pg_port_sweep_spec* spec, uint32_t* out_codes, uint32_t* out_open,
                              uint32_t* out_words, int flags);

/* ---- reachability diff: the cells two audit results differ in, on the device --------------
 * "What did this policy change open or close?" pg_reach_matrix (out_packed) and pg_reach_ports
 * (out_codes) write one layout: 2 bits per cell, 16 cells per word, rows of row_words =
 * pg_reach_row_words(n_cols) words, padding zero -- a matrix has n_svc * n_src rows of n_dst
 * cells, a sweep n_src * n_dst rows of K cells. pg_reach_diff compares two such results of one
 * shape on the device, so neither is copied to the host: typically the live engine's and that of
 * a staging engine with the candidate policy (the two inputs may come from different contexts on
 * the same device; ctx only names the device and its launch knobs).
 *   A cell is selected when its two ConnActions differ and bit (4 * before + after) of
 *   spec->transitions is set; the four diagonal bits are ignored. PG_DIFF_OPENED selects what
 *   became ALLOW, PG_DIFF_CLOSED what stopped being ALLOW.
 *   *n_changes   host, required: the number of selected cells; it may exceed spec->cap
 *   changes      device, optional, spec->cap entries: the first min(*n_changes, cap) selected
 *                cells in ascending (row, column) order; entries past that are not written. Null,
 *                or cap == 0: count only
 *   row_changes  device, optional, n_rows words: the selected cells of every row (every row is
 *                written)
 *   trans        host, optional: trans[4 * b + a] = the cells with ConnAction b before and a
 *                after, over ALL cells whatever `transitions` selects, the diagonal included: the
 *                16 values sum to n_rows * n_cols
 * The padding bits of a row's last word are never compared (they are masked, not trusted). Two
 * port sweeps are comparable only over the same partition lo[] (pg_port_intervals equal on both
 * engines); the call cannot check that. The call reads no table and triggers no compile, and it
 * never touches the hit counters or their snapshots. It enqueues on hip_stream and synchronises
 * that stream before it returns, because the count comes back to the host. n_rows == 0: PG_OK,
 * *n_changes = 0, trans zeroed, nothing else written. PG_EINVAL: a null spec, before, after or
 * n_changes; n_cols 0 or above 2^20; n_rows >= 2^32; n_rows * row_words >= 2^32. */
#define PG_DIFF_ALL    0xFFFFu
#define PG_DIFF_OPENED 0x4044u   /* before != ALLOW, after == ALLOW: bits 2, 6, 14 */
#define PG_DIFF_CLOSED 0x0B00u   /* before == ALLOW, after != ALLOW: bits 8, 9, 11 */
typedef struct pg_reach_change {
    uint32_t row;    /* (v * n_src + i) of a matrix, (i * n_dst + j) of a port sweep */
    uint32_t cell;   /* bits 19-0 column (dst j / interval k), 29-28 ConnAction before, 31-30 after */
} pg_reach_change;
typedef struct pg_reach_diff_spec {
    const uint32_t* before;  /* device, n_rows * pg_reach_row_words(n_cols) words */
    const uint32_t* after;   /* device, same shape */
    uint64_t n_rows;
    uint32_t n_cols;         /* 1 .. 2^20 */
    uint32_t transitions;    /* bit (4 * before + after) set: that transition is selected */
    uint64_t cap;            /* entries `changes` can hold */
} pg_reach_diff_spec;
int pg_reach_diff(pg_ctx* ctx, const pg_reach_diff_spec* spec, pg_reach_change* changes, uint32_t* row_changes,
                  uint64_t* n_changes, uint64_t trans[16], void* hip_stream);
/* TESTS ONLY -- never on the audit path: pg_reach_diff's per-word code (diff.hpp, the functions the
 * kernels call) on the host; before, after, changes and row_changes are host arrays. Does not touch
 * the device. */
int pg_debug_reach_diff_host(pg_ctx* ctx, const pg_reach_diff_spec* spec, pg_reach_change* changes,
                             uint32_t* row_changes, uint64_t* n_changes, uint64_t trans[16]);
/* TESTS ONLY: how a pg_reach_diff over n_words = n_rows * row_words words is cut under this context's
 * knobs (blocks_per_cu), from the one function the launch itself uses (diff.hpp diff_plan): the tile
 * (words a workgroup takes per step), the workgroups, and the words of the contiguous chunk each one
 * owns (a multiple of the tile). Queries the device's size and the kernels' occupancy; launches
 * nothing. */
int pg_debug_reach_diff_plan(pg_ctx* ctx, uint64_t n_words, uint32_t* tile_words, uint32_t* grid,
                             uint64_t* chunk_words);

/* ---- reachability closure: multi-hop reach and hop counts, on the device -------------------
 * "If this pod is compromised, what can the attacker get to by hopping through the pods it
 * reaches, and in how many hops?" The input is a pg_reach_matrix out_packed taken with the SAME
 * end-point list on both sides (n_src == n_dst == n), which stays on the device.
 *   Edge: i -> j when some selected slice v holds PG_CONN_ALLOW in cell (v, i, j). Cell (i, i) is a
 *   cell like any other: there is no implicit self-reach.
 *   hops(i, j): the least k >= 1 for which a path of k edges leads from i to j; hops(i, i) is the
 *   shortest cycle through i. Cell (i, j) is reachable when such a k exists and, with max_hops != 0,
 *   k <= max_hops.
 *   out_packed  device, required, n rows of pg_reach_row_words(n) words in the audits' layout:
 *               PG_CONN_ALLOW in the reachable cells, PG_CONN_DENY_SYN in all others, the padding
 *               bits of a row's last word zero. A valid before / after of pg_reach_diff with n_rows
 *               = n_cols = n ("what did this change open transitively"). With max_hops = 1 it is the
 *               one-hop graph.
 *   out_hops    device, optional, n * n uint16_t, row-major: hops(i, j), 0 for cells that are not
 *               reachable; every cell is written (n <= 2^15: the count always fits)
 *   out_count   device, optional, n words: the reachable cells of each row -- the blast radius of
 *               end point i
 *   result      host, required
 * The padding bits of the input rows are masked, never trusted. Duplicate end points are just equal
 * rows and columns. Like pg_reach_diff the call reads no table and triggers no compile, and it
 * never touches the hit counters or their snapshots; ctx only names the device and its launch
 * knobs. It enqueues on hip_stream, one launch per level, and synchronises that stream, because the
 * counts come back to the host. n == 0: PG_OK, *result zeroed, nothing else written. PG_EINVAL
 * (pg_last_error says which): a null spec, matrix, out_packed or result; n above 2^15; n_svc 0 or
 * above 4096. An all-zero svc_select is valid and gives the empty graph. PG_ENOMEM: the scratch
 * allocation (four n x n bit matrices) failed. */
typedef struct pg_reach_closure_spec {
    const uint32_t* matrix;   /* device: n_svc * n rows of pg_reach_row_words(n) words */
    uint32_t n;               /* end points, 1 .. 2^15 */
    uint32_t n_svc;           /* slices of the matrix, 1 .. 4096 */
    const uint8_t* svc_select;/* host, optional, n_svc bytes: non-zero = this slice contributes edges; NULL = all */
    uint32_t max_hops;        /* 0 = until nothing new is found; k = paths of at most k edges */
} pg_reach_closure_spec;
typedef struct pg_reach_closure_result {   /* host */
    uint32_t levels;          /* the largest hop count assigned to any cell (0: no edge) */
    uint64_t n_edges;         /* cells of the one-hop graph */
    uint64_t n_reachable;     /* cells of the closure */
} pg_reach_closure_result;
int pg_reach_closure(pg_ctx* ctx, const pg_reach_closure_spec* spec, uint32_t* out_packed, uint16_t* out_hops,
                     uint32_t* out_count, pg_reach_closure_result* result, void* hip_stream);
/* TESTS ONLY -- never on the audit path: pg_reach_closure's per-word code (closure.hpp, the
 * functions the kernels call) on the host, level by level; matrix, out_packed, out_hops and
 * out_count are host arrays. Does not touch the device. */
int pg_debug_reach_closure_host(pg_ctx* ctx, const pg_reach_closure_spec* spec, uint32_t* out_packed, uint16_t* out_hops,
                                uint32_t* out_count, pg_reach_closure_result* result);
/* TESTS ONLY: how one level of a pg_reach_closure over n end points is cut, from the one function
 * the launch itself uses (closure.hpp closure_plan): the rows and columns of the output a workgroup
 * owns and the workgroups of a level. Launches nothing. */
int pg_debug_reach_closure_plan(pg_ctx* ctx, uint32_t n, uint32_t* tile_rows, uint32_t* tile_cols, uint32_t* grid);

/* ---- reachability groups: a matrix summed into (src group, dst group) pairs, on the device ---
 * "Can anything in dev reach anything in prod on 5432? Is frontend -> api fully open or only
 * partly?" The input is a pg_reach_matrix out_packed, which stays on the device in its 2 bits per
 * cell; every src and every dst end point is given a group (a namespace, a deployment, a label
 * set) or PG_GROUP_SKIP.
 *   out_counts  device, required, n_svc * n_src_groups * n_dst_groups * 4 uint64_t: entry
 *               ((v * n_src_groups + gs) * n_dst_groups + gd) * 4 + c is the number of cells (v, i, j)
 *               with src_group[i] == gs, dst_group[j] == gd and ConnAction c. Every entry is written,
 *               zeros included (the call clears the array on the stream first). Integer sums: exact,
 *               and the same on every run.
 *   out_packed  device, optional: the PG_GROUPS_* status of every (v, gs, gd) in the audits' layout,
 *               n_svc * n_src_groups rows of pg_reach_row_words(n_dst_groups) words, cell gd in bits
 *               [2 * (gd & 15), 2 * (gd & 15) + 1] of word gd / 16, the padding bits of a row's last
 *               word zero. A valid before / after of pg_reach_diff with n_cols = n_dst_groups: the
 *               diff of two summaries lists the group pairs whose status a policy change moved.
 *               PG_GROUPS_ALL equals PG_CONN_ALLOW, so pg_reach_closure over a square summary
 *               follows the fully open pairs.
 * Any assignment of ids is allowed: not contiguous, not sorted, groups without members, every end
 * point its own group. A pod that belongs to two groups is listed twice in the end-point list that
 * pg_reach_matrix was given. The padding bits of the input rows are masked, never trusted. Like
 * pg_reach_diff the call reads no table and triggers no compile, and it never touches the hit
 * counters or their snapshots; ctx only names the device and its launch knobs. It copies the two
 * host arrays in, enqueues in order on hip_stream and synchronises that stream before it returns.
 * n_svc, n_src or n_dst zero: PG_OK, out_counts cleared and out_packed all PG_GROUPS_EMPTY (the
 * matrix may then be null); with a group count of zero as well, nothing is written. PG_EINVAL
 * (pg_last_error says which argument, and for a bad id which index): a null spec, matrix or
 * out_counts; a null src_group / dst_group where that side is not empty; a side above 2^20; n_svc
 * above 4096; a group count of 0 or above 4096; n_svc * n_src_groups * n_dst_groups >= 2^30; a group
 * id that is neither below its count nor PG_GROUP_SKIP. PG_ENOMEM: the scratch allocation (the
 * sorted rows and the ids) failed. */
#define PG_GROUP_SKIP 0xFFFFFFFFu   /* an end point that belongs to no group: its row / column is counted nowhere */
enum { PG_GROUPS_NONE = 0,   /* the pair has cells, none of them ALLOW            */
       PG_GROUPS_SOME = 1,   /* some cells ALLOW, some not                         */
       PG_GROUPS_ALL = 2,    /* every cell ALLOW (same value as PG_CONN_ALLOW)     */
       PG_GROUPS_EMPTY = 3 };/* no cell: one of the two groups has no member       */
typedef struct pg_reach_groups_spec {
    const uint32_t* matrix;      /* device: a pg_reach_matrix out_packed, n_svc * n_src rows of pg_reach_row_words(n_dst) words */
    uint32_t n_svc, n_src, n_dst;
    const uint32_t* src_group;   /* host, n_src entries: < n_src_groups, or PG_GROUP_SKIP */
    const uint32_t* dst_group;   /* host, n_dst entries: < n_dst_groups, or PG_GROUP_SKIP */
    uint32_t n_src_groups, n_dst_groups;   /* 1 .. 4096 each */
} pg_reach_groups_spec;
int pg_reach_groups(pg_ctx* ctx, const pg_reach_groups_spec* spec, uint64_t* out_counts, uint32_t* out_packed,
                    void* hip_stream);
/* TESTS ONLY -- never on the audit path: pg_reach_groups's per-word code (groups.hpp, the functions
 * the kernels call) on the host, work item by work item; matrix, out_counts and out_packed are host
 * arrays. Does not touch the device. */
int pg_debug_reach_groups_host(pg_ctx* ctx, const pg_reach_groups_spec* spec, uint64_t* out_counts, uint32_t* out_packed);
/* TESTS ONLY: how a pg_reach_groups over rows of n_dst cells is cut, from the one function the
 * launch itself uses (groups.hpp groups_plan): the column words of a work item's tile and the most
 * rows of one src group it walks between two flushes. Launches nothing. */
int pg_debug_reach_groups_plan(pg_ctx* ctx, uint32_t n_dst, uint32_t* tile_words, uint32_t* chunk_rows);

/* ---- reachability paths: shortest attack paths and choke points, on the device -------------
 * "Pod A gets to the database in 3 hops -- through which pods? Which pod do most of those paths pass
 * through?" The input is a pg_reach_closure out_hops (n x n uint16_t, row-major, 0 = not reachable),
 * which stays on the device; a matrix taken with max_hops = k is valid, cells beyond k are simply
 * unreachable. edge(a, b) <=> hops(a, b) == 1.
 *   Path of a query (i, j), d = hops(i, j): none when d == 0; else p_0 = i .. p_d = j with, for t = d,
 *   d - 1, .., 2, p_{t-1} = the least k with hops(i, k) == t - 1 and hops(k, p_t) == 1 (the "least
 *   predecessor": it depends on (i, p_t) only, so the paths of one src form a tree). i == j asks for
 *   the shortest cycle through i and is walked the same way. The intermediates p_1 .. p_{d-1} are
 *   pairwise distinct and differ from i and j.
 *   Over an input that no closure wrote, a step may find no k: the query is *broken* -- out_len 0,
 *   its nodes row all 0xFFFF, counted in n_broken; out_via is then unspecified. On any input the
 *   call ends and stays inside its arrays.
 *   out_len    device, required, n_queries uint16_t at the queries' own positions: d, and 0 for a
 *              query that is unreachable or broken
 *   out_nodes  device, optional, n_queries rows of max_len + 1 uint16_t: p_0 .. p_d, then 0xFFFF. A
 *              path with d > max_len is *too long*: its row is all 0xFFFF, and it still counts in
 *              out_len and out_via. Every entry of every row is written
 *   out_via    device, optional, n words: out_via[k] = the queries whose path has k among its
 *              intermediates -- the choke points. Every word is written (the call clears the array
 *              on the stream first). Integer sums: exact, and the same on every run
 *   result     host, required
 * Duplicate queries are answered each at its position. Like pg_reach_closure the call reads no table
 * and triggers no compile, and it never touches the hit counters or their snapshots; ctx only names
 * the device and its launch knobs. It sorts the queries by src on the host, copies them in, enqueues
 * in order on hip_stream (the transposed edge bits of hops into scratch, then the walk) and
 * synchronises that stream. n_queries == 0: PG_OK, *result zeroed, out_via cleared when given,
 * nothing else written (with n == 0 as well, nothing on the device). PG_EINVAL (pg_last_error says
 * which argument, and for a bad id which index): a null spec, hops, out_len or result; a null src or
 * dst with queries; n above 2^15; n_queries above 2^24; an id >= n; with out_nodes, max_len 0 or above
 * 2^15, or n_queries * (max_len + 1) >= 2^32. PG_ENOMEM: the scratch allocation (n x n bits and the
 * sorted queries) failed. */
typedef struct pg_reach_paths_spec {
    const uint16_t* hops;   /* device, n * n: a pg_reach_closure out_hops; 2-B aligned, nothing more assumed */
    uint32_t n;             /* end points, 1 .. 2^15 */
    const uint32_t* src;    /* host, n_queries entries, each < n; duplicates allowed, any order */
    const uint32_t* dst;    /* host, likewise */
    uint64_t n_queries;     /* 0 .. 2^24 */
    uint32_t max_len;       /* with out_nodes: the longest path (edges) that is written, 1 .. 2^15 */
} pg_reach_paths_spec;
typedef struct pg_reach_paths_result {   /* host */
    uint64_t n_found;       /* queries with a path (out_len != 0) */
    uint64_t n_unreachable; /* hops(i, j) == 0 */
    uint64_t n_too_long;    /* found, but longer than max_len: a subset of n_found; 0 without out_nodes */
    uint64_t n_broken;      /* n_found + n_unreachable + n_broken == n_queries */
    uint64_t n_via;         /* sum of out_via = intermediates over all found paths */
    uint32_t longest;       /* largest out_len */
} pg_reach_paths_result;
int pg_reach_paths(pg_ctx* ctx, const pg_reach_paths_spec* spec, uint16_t* out_len, uint16_t* out_nodes,
                   uint32_t* out_via, pg_reach_paths_result* result, void* hip_stream);
/* TESTS ONLY -- never on the audit path: pg_reach_paths's per-word code, partition and plan
 * (paths.hpp, the functions the kernels and the launch call) on the host, work item by work item;
 * hops, out_len, out_nodes and out_via are host arrays. Does not touch the device. */
int pg_debug_reach_paths_host(pg_ctx* ctx, const pg_reach_paths_spec* spec, uint16_t* out_len, uint16_t* out_nodes,
                              uint32_t* out_via, pg_reach_paths_result* result);
/* TESTS ONLY: how a pg_reach_paths over n end points is cut, from the one function the launch itself
 * uses (paths.hpp paths_plan): the most queries of one src a work item holds, and the most LDS a
 * workgroup takes (the staged row of hops, the counters and, where they fit, the out_via counts).
 * Launches nothing. */
int pg_debug_reach_paths_plan(pg_ctx* ctx, uint32_t n, uint32_t* chunk_queries, uint32_t* lds_bytes);

/* ---- reachability classes: the end points the policy treats identically, on the device -----
 * "Which pods does the policy treat as one role, and which replica differs from its siblings?" The
 * input is a pg_reach_matrix out_packed (n_svc * n_src rows of pg_reach_row_words(n_dst) words), which
 * stays on the device in its 2 bits per cell.
 *   Equality: src end points i, i' are equal when cell(v, i, j) == cell(v, i', j) for every slice v and
 *   every j; dst end points j, j' are equal when cell(v, i, j) == cell(v, i, j') for every v and i. All
 *   four ConnAction codes count, not only ALLOW. A duplicate end point is an equal end point.
 *   Classes: the equivalence classes of those relations, by equality and not by hash: the call
 *   compares 64-bit signatures first and then checks every candidate cell for cell, so the result is
 *   right even when two different signatures share a hash.
 *   Numbering by first appearance: the class of the least end point not yet classed gets the next id,
 *   from 0. So class[0] == 0, the representatives (the least members) ascend, and the ids depend on
 *   nothing but the input.
 *   out_src_class  device, optional, n_src words: the class of every src end point
 *   out_dst_class  device, optional, n_dst words. At least one of the two is given; a side that is not
 *                  asked for is not computed
 *   out_src_rep    device, optional, capacity n_src words: the first n_src_classes entries are each
 *   out_dst_rep    class's least member; entries past that are not written. Likewise n_dst /
 *                  n_dst_classes. Ignored for a side whose class output is null
 *   out_quotient   device, optional, needs both class outputs; capacity that of the input, n_svc *
 *                  n_src * pg_reach_row_words(n_dst) words. The first n_svc * n_src_classes *
 *                  pg_reach_row_words(n_dst_classes) words are the matrix of the representatives in
 *                  the audits' layout: cell (v, cs, cd) = cell(v, src_rep[cs], dst_rep[cd]), the
 *                  padding bits of a row's last word zero; nothing past that is written. A valid
 *                  before / after of pg_reach_diff, and what pg_reach_groups over the two class
 *                  arrays gives as the single non-zero code of every pair
 *   result         host, required
 * The padding bits of the input rows are masked, never trusted. Like pg_reach_diff the call reads no
 * table and triggers no compile, and it never touches the hit counters or their snapshots; ctx only
 * names the device and its launch knobs ("blocks_per_cu", "classes_hash_bits"). It enqueues on
 * hip_stream and synchronises it once per pass: the signatures (8 bytes per end point) and the marks
 * of the equality check come back to the host, which picks the candidates; the matrix is read on the
 * device only. n_svc, n_src or n_dst zero: PG_OK, *result zeroed, nothing else written (the matrix
 * may then be null). PG_EINVAL (pg_last_error says which): a null spec, matrix or result; both class
 * outputs null; out_quotient with a class output missing; a side above 2^20; n_svc above 4096; n_svc
 * * n_src * row_words >= 2^32. PG_ENOMEM: the scratch allocation (signatures, leaders, marks) failed. */
typedef struct pg_reach_classes_spec {
    const uint32_t* matrix;   /* device: a pg_reach_matrix out_packed, n_svc * n_src rows of pg_reach_row_words(n_dst) words */
    uint32_t n_svc, n_src, n_dst;
} pg_reach_classes_spec;
typedef struct pg_reach_classes_result {   /* host */
    uint32_t n_src_classes;   /* 0 for a side that was not asked for */
    uint32_t n_dst_classes;
    uint32_t rounds;          /* the most passes of the equality check either side needed: 1 unless different
                                 signatures shared a hash; 0 on empty input */
} pg_reach_classes_result;
int pg_reach_classes(pg_ctx* ctx, const pg_reach_classes_spec* spec, uint32_t* out_src_class, uint32_t* out_dst_class,
                     uint32_t* out_src_rep, uint32_t* out_dst_rep, uint32_t* out_quotient,
                     pg_reach_classes_result* result, void* hip_stream);
/* TESTS ONLY -- never on the audit path: pg_reach_classes's per-word code, signatures, rounds and plan
 * (classes.hpp, the functions the kernels and the launch call) on the host, work item by work item;
 * matrix and every output are host arrays. Does not touch the device. */
int pg_debug_reach_classes_host(pg_ctx* ctx, const pg_reach_classes_spec* spec, uint32_t* out_src_class,
                                uint32_t* out_dst_class, uint32_t* out_src_rep, uint32_t* out_dst_rep,
                                uint32_t* out_quotient, pg_reach_classes_result* result);
/* TESTS ONLY: how the column passes of a pg_reach_classes over rows of n_dst cells are cut, from the
 * one function the launch itself uses (classes.hpp classes_plan): the column words of a work item's
 * tile, and the rows (of the n_svc * n_src) of a chunk of the dst signatures and of the dst check.
 * Launches nothing. */
int pg_debug_reach_classes_plan(pg_ctx* ctx, uint32_t n_dst, uint32_t* tile_words, uint32_t* chunk_rows,
                                uint32_t* check_rows);

/* ---- reachability zones: mutually reachable end points and their graph, on the device -------
 * "Which end points can all reach each other, and how do those zones sit relative to one another?" The
 * input is a pg_reach_closure out_packed (n rows of pg_reach_row_words(n) words, 2 bits per cell),
 * which stays on the device.
 *   R(i, j): cell (i, j) holds PG_CONN_ALLOW; every other code counts as "no". Cell (i, i) is a cell
 *   like any other.
 *   Mutual reach M(i, j) = R(i, j) and R(j, i). label(i) = the least member of {i} u { j : M(i, j) }.
 *   Over a full closure (max_hops == 0) R is transitive, so label(i) is the least member of i's
 *   strongly connected component of the ALLOW graph -- a lateral-movement zone: it falls as a whole
 *   when one member does. An end point that lies on no cycle is a zone of its own.
 *   Zones: the distinct values of label[], ascending, get the ids 0, 1, ... (numbering by first
 *   appearance, as in pg_reach_classes): zone[0] == 0, the representatives (the least members) ascend,
 *   and the ids depend on nothing but the input.
 *   Any input is defined -- a max_hops-bounded closure, a one-hop matrix, random words -- and the call
 *   stays inside its arrays on it: where R is not transitive the labels are still the formula above,
 *   and n_broken counts the end points i with label(label(i)) != label(i). It is 0 on every full
 *   closure. Duplicate end points are equal rows and columns; they share a zone only if that pod
 *   reaches itself.
 *   out_zone        device, required, n words: the zone id of every end point
 *   out_rep         device, optional, capacity n words: the first n_zones entries are each zone's least
 *                   member; nothing past that is written
 *   out_size        device, optional, capacity n: the first n_zones entries are the number of i with
 *                   out_zone[i] == z. Integer counts: exact, and the same on every run
 *   out_reaches     device, optional, capacity n each: for zone z with representative r the first
 *   out_reached_by  n_zones entries are the number of j with R(r, j) -- the end points the zone
 *                   reaches, its blast radius -- and the number of i with R(i, r), its exposure
 *   out_dag         device, optional, needs out_rep; capacity n * pg_reach_row_words(n) words. The first
 *                   n_zones * pg_reach_row_words(n_zones) words are the zone graph in the audits'
 *                   layout: cell (a, b) = PG_CONN_ALLOW iff R(rep[a], rep[b]), else PG_CONN_DENY_SYN, the
 *                   padding bits of a row's last word zero; nothing past that is written. The
 *                   diagonal cell (z, z) is ALLOW exactly for a zone whose members lie on a cycle. A
 *                   valid before / after of pg_reach_diff where two graphs have one size
 *   result          host, required
 * The padding bits of the input rows are masked, never trusted. Like pg_reach_closure the call reads
 * no table and triggers no compile, and it never touches the hit counters or their snapshots; ctx only
 * names the device and its launch knobs ("blocks_per_cu"). It enqueues on hip_stream -- the bits of R
 * and of its transpose into scratch, the labels, the numbering, the zone graph, whose launch takes
 * its geometry from device memory -- and synchronises that stream once, at the end, because the
 * counts come back to the host. n == 0: PG_OK, *result zeroed, nothing else written (the matrix may
 * then be null). PG_EINVAL (pg_last_error says which): a null spec, matrix, out_zone or result; out_dag
 * without out_rep; n above 2^15. PG_ENOMEM: the scratch allocation (two n x n bit matrices and a few
 * words per end point) failed. */
typedef struct pg_reach_zones_spec {
    const uint32_t* matrix;   /* device: a pg_reach_closure out_packed, n rows of pg_reach_row_words(n) words; 4-B aligned, nothing more assumed */
    uint32_t n;               /* end points, 0 .. 2^15 */
} pg_reach_zones_spec;
typedef struct pg_reach_zones_result {   /* host */
    uint32_t n_zones;
    uint32_t n_cyclic;        /* zones with R(rep, rep): their members lie on a cycle */
    uint32_t n_multi;         /* zones of more than one member */
    uint32_t largest;         /* the largest out_size */
    uint32_t n_broken;        /* end points with label(label(i)) != label(i): 0 where R is transitive */
} pg_reach_zones_result;
int pg_reach_zones(pg_ctx* ctx, const pg_reach_zones_spec* spec, uint32_t* out_zone, uint32_t* out_rep, uint32_t* out_size,
                   uint32_t* out_reaches, uint32_t* out_reached_by, uint32_t* out_dag, pg_reach_zones_result* result,
                   void* hip_stream);
/* TESTS ONLY -- never on the audit path: pg_reach_zones's per-word code and plan (zones.hpp, the
 * functions the kernels and the launch call) on the host, work item by work item; matrix and every
 * output are host arrays. Does not touch the device. */
int pg_debug_reach_zones_host(pg_ctx* ctx, const pg_reach_zones_spec* spec, uint32_t* out_zone, uint32_t* out_rep,
                              uint32_t* out_size, uint32_t* out_reaches, uint32_t* out_reached_by, uint32_t* out_dag,
                              pg_reach_zones_result* result);
/* TESTS ONLY: how a pg_reach_zones over n end points is cut, from the one function the launch itself
 * uses (zones.hpp zones_plan): the rows and columns of a transpose tile and the tiles there are, the
 * rows of a label work item and the work items there are. Launches nothing. */
typedef struct pg_reach_zones_plan {
    uint32_t tile_rows, tile_cols;   /* cells of the matrix one transpose tile covers */
    uint32_t row_tiles, col_tiles;   /* bits_grid = row_tiles * col_tiles */
    uint32_t bits_grid;
    uint32_t label_rows, label_grid; /* rows of a label work item; work items */
    uint32_t dag_grid;               /* the most workgroups the zone graph can need: one per zone */
} pg_reach_zones_plan;
int pg_debug_reach_zones_plan(pg_ctx* ctx, uint32_t n, pg_reach_zones_plan* plan);

/* ---- reachability dominators: the end points every attack path must cross, on the device -----
 * "The attacker holds these pods; which single pod, if quarantined, cuts them off from the most
 * targets, and which pods stand between them and v on every route?" The input has pg_reach_closure's
 * form: a pg_reach_matrix out_packed taken with one end-point list on both sides (n_svc slices of n
 * rows of pg_reach_row_words(n) words), which stays on the device, an optional svc_select, and a host
 * list of entry end points E, the foothold.
 *   Edge i -> j: some selected slice holds PG_CONN_ALLOW in cell (i, j) -- pg_reach_closure's rule. Cell
 *   (i, i) is a cell like any other.
 *   v is reached when v is in E, or some walk of one or more edges leads from a member of E to v.
 *   k dominates a reached v when every walk from any member of E to v contains k; the walk of no
 *   edges counts when v is in E. So v dominates itself, an entry is dominated by itself only, a
 *   single entry dominates every reached end point, and an unreached end point has no dominators.
 *   Dom(v) is a chain under dominance: |Dom(.)| strictly increases along it.
 *   idom(v): the k in Dom(v) \ {v} with |Dom(k)| == |Dom(v)| - 1; exactly one when Dom(v) \ {v} is
 *   not empty, none otherwise.
 *   cut[k]: the number of v != k with k in Dom(v) -- the end points the attacker loses when k alone is
 *   quarantined.
 *   out_dom   device, optional, n rows of pg_reach_row_words(n) words in the audits' layout: cell (v, k)
 *             holds PG_CONN_ALLOW iff k is in Dom(v), else PG_CONN_DENY_SYN; the padding bits of a row's
 *             last word are zero and every word is written. A valid before / after of pg_reach_diff
 *             (which lists the choke points a policy change created or removed) and a valid input of
 *             pg_reach_groups
 *   out_idom  device, optional, n uint16_t, each written: idom(v), or 0xFFFF where there is none -- the
 *             entries, the unreached end points, and the end points with no strict dominator
 *   out_cut   device, optional, n words, each written. Integer sums: exact, and the same on every run
 *   result    host, required. All three outputs may be null: the result alone is an answer
 * The sets are the least fixed point of Avoid(v) = (U over edges p -> v of Avoid(p)) \ {v} with
 * Avoid(e) = all \ {e} fixed for e in E, where Avoid(v) is the set of k that some walk from E to v
 * does not contain; Dom(v) is its complement for a reached v. result->rounds counts the rounds r >= 1
 * of the synchronous iteration Avoid_r+1(v) = Avoid_r(v) | ((U Avoid_r(p)) \ {v}) in which some set
 * grew, reachedness carried as one more column that is set in the entries' rows: it depends on nothing
 * but the input.
 * The padding bits of the input rows are masked, never trusted. Like pg_reach_closure the call reads
 * no table and triggers no compile, and it never touches the hit counters or their snapshots; ctx only
 * names the device and its launch knobs ("blocks_per_cu"). It enqueues on hip_stream -- the edges
 * transposed into scratch, one launch per round, the finish -- and synchronises that stream after
 * every round, because the host reads the running count back to see whether anything grew, and at
 * the end. On any input the call ends and stays inside its arrays. n == 0: PG_OK, *result zeroed,
 * nothing else written (the matrix may then be null). n_entry == 0 or an all-zero svc_select is valid:
 * nothing, or only E, is reached. PG_EINVAL (pg_last_error names the argument, and for a bad id its
 * index): a null spec or result; a null matrix with n > 0; a null entry with n_entry > 0; n or n_entry
 * above 2^15; n_svc 0 or above 4096; an entry id >= n. PG_ENOMEM: the scratch allocation (four n x n
 * bit matrices and a few words per end point) failed. */
typedef struct pg_reach_dominators_spec {
    const uint32_t* matrix;     /* device: n_svc * n rows of pg_reach_row_words(n) words; 4-B aligned, nothing more assumed */
    uint32_t n;                 /* end points, 0 .. 2^15 */
    uint32_t n_svc;             /* 1 .. 4096 */
    const uint8_t* svc_select;  /* host, optional, as in pg_reach_closure_spec */
    const uint32_t* entry;      /* host, n_entry ids, each < n; duplicates allowed, any order */
    uint32_t n_entry;           /* 0 .. 2^15; 0 = nothing is reached */
} pg_reach_dominators_spec;
typedef struct pg_reach_dominators_result {   /* host */
    uint32_t n_reached;   /* entries included */
    uint32_t n_chokes;    /* end points outside E with cut > 0 */
    uint32_t top;         /* the least end point outside E with the largest cut; 0xFFFFFFFF when n_chokes == 0 */
    uint32_t top_cut;     /* its cut, 0 when none */
    uint32_t depth;       /* max over v of |Dom(v)| - 1: the longest chain of strict dominators */
    uint32_t rounds;      /* as defined above */
} pg_reach_dominators_result;
int pg_reach_dominators(pg_ctx* ctx, const pg_reach_dominators_spec* spec, uint32_t* out_dom, uint16_t* out_idom,
                        uint32_t* out_cut, pg_reach_dominators_result* result, void* hip_stream);
/* TESTS ONLY -- never on the audit path: pg_reach_dominators's per-word code and plan (dominators.hpp,
 * the functions the kernels and the launch call) on the host, round by round; matrix and every output
 * are host arrays. Does not touch the device. */
int pg_debug_reach_dominators_host(pg_ctx* ctx, const pg_reach_dominators_spec* spec, uint32_t* out_dom, uint16_t* out_idom,
                                   uint32_t* out_cut, pg_reach_dominators_result* result);
/* TESTS ONLY: how a pg_reach_dominators over n end points is cut, from the one function the launch
 * itself uses (dominators.hpp dom_plan): a round's lane words, tile and grid, the edge / transpose
 * tiles, the cut tiles and the per-row grid of the finish. Launches nothing. */
typedef struct pg_reach_dominators_plan {
    uint32_t lane_words;                         /* adjacent bit-words of a row a lane owns in a round: 1, 2 or 4 */
    uint32_t tile_rows, tile_cols;               /* cells of the sets one workgroup of a round owns */
    uint32_t row_tiles, col_tiles, round_grid;   /* round_grid = row_tiles * col_tiles */
    uint32_t t_rows, t_cols;                     /* cells of the edge matrix one transpose tile covers */
    uint32_t t_row_tiles, t_col_tiles, t_grid;   /* t_grid = t_row_tiles * t_col_tiles */
    uint32_t cut_rows, cut_cols;                 /* cells of Dom one cut tile covers */
    uint32_t cut_row_tiles, cut_col_tiles, cut_grid;
    uint32_t finish_grid;                        /* the most workgroups the size and idom kernels can need: one per row */
} pg_reach_dominators_plan;
int pg_debug_reach_dominators_plan(pg_ctx* ctx, uint32_t n, pg_reach_dominators_plan* plan);

/* ---- reachability cut: the fewest end points that cut entries from targets, on the device -----
 * "The attacker holds these pods and wants those pods. What is the smallest set of pods I must
 * quarantine so that no route is left, and how many independent routes are there today?" -- the
 * minimum vertex cut between an entry set E and a target set T, which pg_reach_dominators sees only
 * at size one. The input has pg_reach_dominators' form: a square pg_reach_matrix out_packed on the
 * device (n_svc slices of n rows of pg_reach_row_words(n) words), an optional svc_select, host lists
 * of entry and target end points, and max_cut.
 *   Edge i -> j: some selected slice holds PG_CONN_ALLOW in cell (i, j) -- pg_reach_closure's rule.
 *   Self edges, edges into members of E and edges out of members of T never matter, and nothing below
 *   sees them.
 *   A set C of end points outside E u T separates when no walk leads from a member of E to a member
 *   of T in the graph without C. The input is inseparable when E n T is not empty or some edge e -> t
 *   joins them directly; n_direct counts the distinct pairs (e, t) with e == t or an edge e -> t.
 *   cut_size is the least |C| over separating C. By Menger's theorem it is the largest number of
 *   E -> T paths that share no end point outside E u T; each has the form e, interior end points
 *   outside E u T, t.
 *   Among the minimum cuts exactly one has a retained region Reach(C) -- the end points reachable from
 *   E without C, E included -- that is contained in that of every other: the near cut, the quarantine
 *   closest to the attacker. Exactly one minimises the region that can still reach T in the same
 *   sense: the far cut, closest to the targets. Both are properties of the graph, not of the algorithm.
 *   In the split graph (v outside E u T becomes v_in -> v_out of capacity 1, edges unbounded), after
 *   any maximum flow: near = { v : v_in is residual-reachable from the source, v_out is not }, far =
 *   { v : v_out residual-reaches the sink, v_in does not }.
 *   max_cut bounds the search: it stops as soon as max_cut + 1 disjoint paths exist. The run is then
 *   capped, and the paths are the proof that no cut of that size exists.
 *   out_cut   device, optional, n bytes of PG_CUT_* flags, each written: the two canonical cuts and
 *             the members of Reach(near) and Reach(far). All zero when the input is inseparable or the
 *             run is capped
 *   out_prev, out_next  device, optional, n uint16_t each, each written: the witness paths. For v
 *             outside E u T on a witness path its predecessor and successor on that path (the
 *             predecessor may be an entry, the successor a target); 0xFFFF everywhere else. An interior
 *             end point is on at most one path; a path starts where out_prev[v] is in E and ends where
 *             out_next[v] is in T. Which maximum set of paths is found is decided by the rules "a level
 *             is one residual arc, the least parent, the least target": the same bytes on every run
 *   result    host, required. All three outputs may be null: the result alone is an answer
 * Shortest augmenting paths, one per search, found level by level over bit sets; after the last
 * search one search back from the sink and two plain searches with each cut removed. result->levels
 * counts the levels of all of them, result->reroutes the residual back arcs on all augmenting paths
 * -- how often a later route displaced an earlier one; both depend on nothing but the input.
 * The padding bits of the input rows are masked, never trusted. Like pg_reach_closure the call reads
 * no table and triggers no compile, and it never touches the hit counters or their snapshots; ctx only
 * names the device and its launch knobs ("blocks_per_cu"). It enqueues on hip_stream and synchronises
 * that stream after every level, because the host reads the level's status back, and at the end. On
 * any input the call ends and stays inside its arrays: at most min(n, max_cut + 1) augmentations of
 * at most 2 n + 2 levels each. n == 0: PG_OK, *result zeroed, nothing else written (the matrix may
 * then be null). An empty E or T or an all-zero svc_select is valid: separable, cut_size 0. PG_EINVAL
 * (pg_last_error names the argument, and for a bad id its index): a null spec or result; a null
 * matrix with n > 0; a null list with a non-zero count; n, n_entry, n_target or max_cut above 2^15;
 * n_svc 0 or above 4096; an id >= n. PG_ENOMEM: the scratch allocation (two n x n bit matrices and a
 * few words per end point) failed. */
#define PG_CUT_NEAR 1u        /* a member of the near cut */
#define PG_CUT_FAR 2u         /* a member of the far cut */
#define PG_CUT_NEAR_REACH 4u  /* reachable from E with the near cut removed, E included */
#define PG_CUT_FAR_REACH 8u   /* reachable from E with the far cut removed, E included */
typedef struct pg_reach_cut_spec {
    const uint32_t* matrix;     /* device: n_svc * n rows of pg_reach_row_words(n) words; 4-B aligned, nothing more assumed */
    uint32_t n;                 /* end points, 0 .. 2^15 */
    uint32_t n_svc;             /* 1 .. 4096 */
    const uint8_t* svc_select;  /* host, optional, as in pg_reach_closure_spec */
    const uint32_t* entry;      /* host, n_entry ids, each < n; duplicates allowed, any order */
    uint32_t n_entry;           /* 0 .. 2^15 */
    const uint32_t* target;     /* host, n_target ids, each < n; duplicates allowed, any order */
    uint32_t n_target;          /* 0 .. 2^15 */
    uint32_t max_cut;           /* 0 .. 2^15: the largest cut looked for */
} pg_reach_cut_spec;
typedef struct pg_reach_cut_result {   /* host */
    uint32_t separable;   /* 0 when the input is inseparable */
    uint32_t capped;      /* 1 when max_cut + 1 disjoint paths exist */
    uint32_t n_direct;    /* as defined above; separable == (n_direct == 0) */
    uint32_t cut_size;    /* 0xFFFFFFFF when the input is inseparable or the run is capped */
    uint32_t n_paths;     /* cut_size; max_cut + 1 when capped; 0 when inseparable */
    uint32_t near_reach;  /* |Reach(near)|, E included; 0 when there is no cut to report */
    uint32_t far_reach;   /* |Reach(far)|, E included; 0 when there is no cut to report */
    uint32_t levels;      /* as defined above */
    uint32_t reroutes;    /* as defined above */
} pg_reach_cut_result;
int pg_reach_cut(pg_ctx* ctx, const pg_reach_cut_spec* spec, uint8_t* out_cut, uint16_t* out_prev, uint16_t* out_next,
                 pg_reach_cut_result* result, void* hip_stream);
/* TESTS ONLY -- never on the audit path: pg_reach_cut's per-word code and plan (cut.hpp, the functions
 * the kernels and the launch call) on the host, level by level; matrix and every output are host
 * arrays. Does not touch the device. */
int pg_debug_reach_cut_host(pg_ctx* ctx, const pg_reach_cut_spec* spec, uint8_t* out_cut, uint16_t* out_prev, uint16_t* out_next,
                            pg_reach_cut_result* result);
/* TESTS ONLY: how a pg_reach_cut over n end points is cut, from the one function the launch itself
 * uses (cut.hpp cut_plan): a level's lane words, workgroup and grid, the edge / transpose tiles and
 * the finish. Launches nothing. */
typedef struct pg_reach_cut_plan {
    uint32_t lane_words;                         /* adjacent bit-words of a row a lane reads per step: 1, 2 or 4 */
    uint32_t level_block, group_nodes;           /* threads of a level's workgroup and the end points it owns */
    uint32_t row_steps, level_grid;              /* steps of 64 * lane_words words that cover a row; workgroups of a level */
    uint32_t t_rows, t_cols;                     /* cells of the edge matrix one transpose tile covers */
    uint32_t t_row_tiles, t_col_tiles, t_grid;   /* t_grid = t_row_tiles * t_col_tiles */
    uint32_t finish_block, finish_grid;          /* the finish: one workgroup */
} pg_reach_cut_plan;
int pg_debug_reach_cut_plan(pg_ctx* ctx, uint32_t n, pg_reach_cut_plan* plan);

/* ---- reachability cost: the cheapest attack paths under per-pod costs, on the device -----------
 * "What is the cheapest way from this pod to the database, given how hard each pod is to take, and
 * which pod do most cheap routes cross?" -- what pg_reach_closure's hops and pg_reach_paths answer
 * when every pod costs the same. The input has pg_reach_dominators' form: a square pg_reach_matrix
 * out_packed on the device (n_svc slices of n rows of pg_reach_row_words(n) words), an optional
 * svc_select, a host list src of n_src source end points (duplicates allowed, any order), a host
 * array weight of n uint16_t, each in 1..65535 -- what it costs to take that end point -- and max_cost.
 *   Edge i -> j: some selected slice holds PG_CONN_ALLOW in cell (i, j) -- pg_reach_closure's rule.
 *   Cell (i, i) is a cell like any other.
 *   cost(s, v) = the least sum of weight[p_t], t = 1..k, over walks s = p_0 -> .. -> p_k = v of k >= 1
 *   edges. The source is already held and costs nothing; cost(s, s) is the cheapest cycle through s
 *   (no implicit self-reach, as in the closure). Cell (s, v) is *reached* when such a walk exists and,
 *   with max_cost != 0, its cost is <= max_cost. Weights are >= 1, so a cheapest walk never repeats
 *   an end point and every cost is <= n * 65535 < 2^31.
 *   base(s, p) = 0 if p == s, else cost(s, p). pred(s, v) = the least p with an edge p -> v, base(s, p)
 *   defined and base(s, p) + weight[v] == cost(s, v) -- the weighted form of pg_reach_paths' least
 *   predecessor; one exists for every reached cell.
 *   The path of (s, v) is v, pred(s, v), pred(s, pred(s, v)), .. and ends at the first predecessor
 *   equal to s (the start, not the cell (s, s)); costs strictly fall along it, so it ends. len(s, v)
 *   = its edges; its intermediates are its end points other than the start and v.
 *   out_cost  device, optional, n_src x n uint32_t: cost, PG_COST_NONE where not reached
 *   out_pred  device, optional, n_src x n uint16_t: pred, PG_COST_NO_PRED where not reached
 *   out_len   device, optional, n_src x n uint16_t: len, 0 where not reached
 *   out_via   device, optional, n uint32_t: out_via[k] = the reached cells (s, v), over all listed
 *             sources with a duplicate source counted twice, whose path has k among its intermediates
 *             -- the weighted choke points. Cleared on the stream first; integer sums: exact, and the
 *             same on every run
 *   result    host, required. All four outputs may be null: the result alone is an answer
 * Every entry of every given array is written. Nothing in *result is a round count: the search is
 * asynchronous inside a workgroup and its rounds are no property of the graph.
 * With every weight 1 and max_cost 0: out_cost is pg_reach_closure's out_hops on the sources' rows
 * (0 <-> PG_COST_NONE), out_len == out_cost, out_pred is pg_reach_paths' predecessor (the end point
 * before v on the path of the query (s, v)), and out_via is pg_reach_paths' out_via over the queries
 * {(s, v) : s listed, every v}.
 * One workgroup runs every round of one source's search inside a single launch, the cost row in LDS
 * where it fits ("cost_lds_bytes"): no launch and no host read per round.
 * The padding bits of the input rows are masked, never trusted. Like pg_reach_closure the call reads
 * no table and triggers no compile, and it never touches the hit counters or their snapshots; ctx only
 * names the device and its launch knobs ("blocks_per_cu", "cost_lds_bytes" -- the result depends on
 * neither). It enqueues on hip_stream and synchronises that stream, because the result comes back. On
 * any input the call ends and stays inside its arrays: a search is bounded by n + 1 rounds, a path by
 * n steps. n == 0 or n_src == 0: PG_OK, *result zeroed, out_via cleared when given and n > 0, nothing
 * else written (the matrix may be null when n == 0). An all-zero svc_select is valid: nothing is
 * reached. PG_EINVAL (pg_last_error names the argument, and for a bad id or weight its index): a
 * null spec or result; a null matrix with n > 0; a null src with n_src > 0 or a null weight with
 * n > 0; n or n_src above 2^15; n_src * n >= 2^28; n_svc 0 or above 4096; a source id >= n; a weight
 * of 0. PG_ENOMEM: the scratch allocation (two n x n bit matrices, the lists and a row per
 * workgroup) failed. */
#define PG_COST_NONE 0xFFFFFFFFu   /* out_cost of a cell that is not reached */
#define PG_COST_NO_PRED 0xFFFFu    /* out_pred of a cell that is not reached */
typedef struct pg_reach_cost_spec {
    const uint32_t* matrix;     /* device: n_svc * n rows of pg_reach_row_words(n) words; 4-B aligned, nothing more assumed */
    uint32_t n;                 /* end points, 0 .. 2^15 */
    uint32_t n_svc;             /* 1 .. 4096 */
    const uint8_t* svc_select;  /* host, optional, as in pg_reach_closure_spec */
    const uint32_t* src;        /* host, n_src ids, each < n; duplicates allowed, any order */
    uint32_t n_src;             /* 0 .. 2^15, n_src * n < 2^28 */
    const uint16_t* weight;     /* host, n weights, each 1 .. 65535 */
    uint32_t max_cost;          /* 0 = no bound */
} pg_reach_cost_spec;
typedef struct pg_reach_cost_result {   /* host */
    uint64_t n_reached;   /* reached cells */
    uint64_t n_via;       /* sum of out_via = sum over the reached cells of (len - 1) */
    uint32_t max_cost;    /* the largest reported cost; 0 when nothing is reached */
    uint32_t longest;     /* the largest len */
} pg_reach_cost_result;
int pg_reach_cost(pg_ctx* ctx, const pg_reach_cost_spec* spec, uint32_t* out_cost, uint16_t* out_pred, uint16_t* out_len,
                  uint32_t* out_via, pg_reach_cost_result* result, void* hip_stream);
/* TESTS ONLY -- never on the audit path: pg_reach_cost's per-word code (cost.hpp, the functions the
 * kernel calls) on the host, source by source; matrix and every output are host arrays. Does not
 * touch the device. */
int pg_debug_reach_cost_host(pg_ctx* ctx, const pg_reach_cost_spec* spec, uint32_t* out_cost, uint16_t* out_pred, uint16_t* out_len,
                             uint32_t* out_via, pg_reach_cost_result* result);
/* TESTS ONLY: how a pg_reach_cost over n end points is laid out under the context's "cost_lds_bytes",
 * from the one function the launch itself uses (cost.hpp cost_plan). Launches nothing. */
typedef struct pg_reach_cost_plan {
    uint32_t lane_words;                         /* adjacent bit-words of a row a lane reads per step: 1, 2 or 4 */
    uint32_t block;                              /* threads of the workgroup that owns one source at a time */
    uint32_t lds_bytes;                          /* its dynamic LDS: two bit vectors, control words, and what is staged */
    uint32_t row_in_lds, weights_in_lds;         /* the cost row (n x 4 B) and the weights (n x 2 B): 1 = staged in LDS */
    uint32_t t_rows, t_cols;                     /* cells of the edge matrix one transpose tile covers */
    uint32_t t_row_tiles, t_col_tiles, t_grid;   /* t_grid = t_row_tiles * t_col_tiles */
} pg_reach_cost_plan;
int pg_debug_reach_cost_plan(pg_ctx* ctx, uint32_t n, pg_reach_cost_plan* plan);

/* ---- observed reachability: a flow log as a reach matrix, on the device -----------------------
 * "Which allowed cells has no flow ever used, and which flows fall on a cell the policy does not
 * allow?" The other audits say what the policy allows; this one folds what the cluster did -- a
 * batch of 5-tuples, device-resident like pg_classify's -- into pg_reach_matrix's layout over the
 * caller's end-point lists and services, so that both answers are existing calls on the device:
 * pg_reach_diff(before = allowed, after = observed) with PG_DIFF_CLOSED lists the allowed cells no
 * flow used, with PG_DIFF_OPENED the cells seen but not allowed; pg_reach_groups over the observed
 * matrix is the per-namespace view.
 *   End points: flow t has the src index set S = { i : src_ip[i] == flows.src_ip[t] } and the dst
 *   index set D likewise. Every duplicate in a list counts.
 *   Services: protocol codes above 3 are read as 3 on both sides, as pg_classify does. Service v
 *   matches flow t when the protocols are equal and, for TCP and UDP only, dst_port is equal; with
 *   PG_OBSERVED_MATCH_SRC_PORT src_port must be equal as well, for TCP and UDP. flows->src_port is
 *   read only with that flag and may otherwise be null. V = the matching services; several services
 *   may share a key.
 *   Status of a flow, the first that applies: S empty PG_OBS_NO_SRC, D empty PG_OBS_NO_DST, V empty
 *   PG_OBS_NO_SVC, otherwise PG_OBS_MATCHED. A matched flow marks every cell of V x S x D.
 *   out_packed     device, required: pg_reach_matrix's out_packed layout exactly, n_svc * n_src rows of
 *                  pg_reach_row_words(n_dst) words. Marked cells hold PG_CONN_ALLOW, all others
 *                  PG_CONN_DENY_SYN, padding bits zero. Without PG_OBSERVED_ACCUMULATE the call clears
 *                  it on the stream first; with it the call ORs into what is there -- the caller
 *                  vouches that an earlier call with the same lists wrote it. A valid before / after
 *                  of pg_reach_diff and input of pg_reach_groups, pg_reach_classes, pg_reach_closure
 *   out_flow       device, optional, n bytes: the status of every flow at its own position
 *   out_svc_flows  device, optional, n_svc u64: the matched flows with v in V; every entry is written.
 *                  Integer sums: exact, and the same on every run
 *   result         host, required
 * Like pg_reach_diff the call reads no table and triggers no compile, and it never touches the hit
 * counters or their snapshots; ctx only names the device and its knobs ("blocks_per_cu",
 * "launch_max_tuples", "observed_lds_bytes", "observed_test_first" -- the result depends on none).
 * The flow arrays need their element's own alignment and nothing more (arrays that all start at
 * 16-B boundaries are read with 16-B loads). Any byte in proto and any port value is valid input; on
 * any input the call ends and stays inside its arrays. It copies the tables built from the lists in,
 * enqueues in order on hip_stream and synchronises it before it returns.
 * n == 0: PG_OK, the outputs cleared as above (out_packed kept with ACCUMULATE), n_cells counted, the
 * other result fields zero; flows may then be null. An empty side: PG_OK, *result zeroed, every flow
 * PG_OBS_NO_SRC or PG_OBS_NO_DST in out_flow, out_svc_flows cleared; out_packed has no words.
 * PG_EINVAL (pg_last_error says which): a null spec, result or out_packed, null flows with n > 0; a
 * null required flow field; a null list of a side that is not empty, or null services; n_svc 0 or
 * above 4096; a side above 2^20; n_svc * n_src * row_words >= 2^32; unknown flag bits. PG_ENOMEM: the
 * scratch allocation (the tables: 12 B per cell of at least twice a list's length, 4 B per end
 * point) failed. */
enum { PG_OBS_MATCHED = 0, PG_OBS_NO_SRC = 1, PG_OBS_NO_DST = 2, PG_OBS_NO_SVC = 3 };
#define PG_OBSERVED_ACCUMULATE     1u  /* out_packed holds an earlier result of the same shape: OR into it, do not clear */
#define PG_OBSERVED_MATCH_SRC_PORT 2u  /* a TCP/UDP flow matches a service only if src_port is equal too */
typedef struct pg_reach_observed_spec {
    const uint32_t* src_ip;   /* host arrays, host-order IPv4, as in pg_reach_spec; duplicates allowed */
    size_t n_src;
    const uint32_t* dst_ip;
    size_t n_dst;
    const pg_service* services; /* host, 1 .. 4096 */
    size_t n_svc;
    uint32_t flags;           /* PG_OBSERVED_* */
} pg_reach_observed_spec;
typedef struct pg_reach_observed_result {   /* host */
    uint64_t n_matched, n_no_src, n_no_dst, n_no_svc;   /* sum == n */
    uint64_t n_cells;                                   /* ALLOW cells of out_packed after the call */
} pg_reach_observed_result;
int pg_reach_observed(pg_ctx* ctx, const pg_reach_observed_spec* spec, const pg_tuple_soa* flows, uint64_t n,
                      uint32_t* out_packed, uint8_t* out_flow, uint64_t* out_svc_flows, pg_reach_observed_result* result,
                      void* hip_stream);
/* TESTS ONLY -- never on the audit path: pg_reach_observed's tables and per-flow code (observed.hpp,
 * the functions the kernel calls) on the host, flow by flow; the flow arrays and every output are
 * host arrays. Does not touch the device. */
int pg_debug_reach_observed_host(pg_ctx* ctx, const pg_reach_observed_spec* spec, const pg_tuple_soa* flows, uint64_t n,
                                 uint32_t* out_packed, uint8_t* out_flow, uint64_t* out_svc_flows,
                                 pg_reach_observed_result* result);
/* TESTS ONLY: how a pg_reach_observed over lists of these lengths is laid out under the context's
 * knobs ("observed_lds_bytes", "blocks_per_cu"), from the one function the launch itself uses
 * (observed.hpp observed_plan). A launch takes tiles of block * vec_flows flows (block on the scalar
 * path), one run of tiles per workgroup. Launches nothing; without a device the grid is that of 256
 * CUs with one workgroup each, the rest is the same. */
typedef struct pg_reach_observed_plan {
    uint32_t src_cap, dst_cap;         /* cells of the address tables: powers of two, at least twice the list */
    uint32_t src_in_lds, dst_in_lds;   /* 1: staged in LDS by every workgroup, 0: probed in HBM */
    uint32_t svc_bytes, lds_bytes;     /* LDS of the service table and the counters; all dynamic LDS */
    uint32_t block, vec_flows;         /* lanes of a workgroup; flows of a lane per step on the vector path */
    uint32_t grid;                     /* the most workgroups of a launch: the resident ones */
} pg_reach_observed_plan;
int pg_debug_reach_observed_plan(pg_ctx* ctx, size_t n_src, size_t n_dst, size_t n_svc, pg_reach_observed_plan* plan);
/* TESTS ONLY: where the address table built over list[0 .. n_list) finds each of n addresses, read
 * off the host table by a plain loop, as pg_debug_endpoint_probe does for the end-point table:
 * out_slot[i] = the cell the probe of ips[i] starts at, out_steps[i] = the cells it reads until it
 * hits the address or an empty cell (1 = the first cell decides), *out_cap = the table's cells (a
 * probe wraps from cell cap - 1 to cell 0). Any output may be null. Tests use it to show that their
 * inputs reach a collision chain or a wrap -- never for an expected value. */
int pg_debug_reach_observed_probe(pg_ctx* ctx, const uint32_t* list, size_t n_list, const uint32_t* ips, uint64_t n,
                                  uint32_t* out_steps, uint32_t* out_slot, uint32_t* out_cap);

/* ---- rule coverage: per-rule histograms of a reach product, on the device --------------------
 * "Which rules do any work over my inventory, which are dead or shadowed, and which rule denies the
 * most pairs?" The product is pg_reach_matrix's (the pg_reach_spec fields: the same end-point
 * resolution, preamble FAILUREs and form A / form B partition of the services), but no cell is
 * written: the call counts, per counter slot (pg_num_counter_slots, pg_slot_info),
 *   out_evals  device, optional, n_slots u64: out_evals[s] = the weighted number of evalACL
 *              evaluations over the product that slot s decided; one count at the "unresolved" slot
 *              per pair that fails the preamble, evaluations of an interface without an ACL at the
 *              "no ACL" slot. Exactly what pg_classify(PG_MODE_CONN, counters) adds to a zeroed
 *              counter array for the product's tuples, each tuple of slice v repeated svc_weight[v]
 *              times
 *   out_cells  device, optional, 4 * n_slots u64: out_cells[4 * s + c] = the weighted number of
 *              cells (v, i, j) whose verdict word is c << 30 | s -- the histogram of pg_reach_matrix's
 *              out_words without writing them. It sums to n_src * n_dst * (the sum of the weights)
 * At least one of the two is given. The call clears them on hip_stream before it adds, so every
 * entry is written, zeros included. Both are integer sums: exact, and the same on every run.
 *   svc_weight host, optional, n_svc: cell and evaluations of slice v count svc_weight[v] times, 0 ..
 *              65536; NULL = every weight 1; 0 = the slice contributes nothing. With the services the
 *              representatives lo[k] of pg_port_intervals and the weights the interval lengths, one
 *              call covers all 65,536 dst ports of a protocol exactly at K evaluations per pair
 *   n_slots    the slot count the caller sized out_evals / out_cells for
 *   result     host, required: n_slots and the layout generation the counts are in
 *              (pg_counter_layout_gen), n_cells = n_src * n_dst * sum of weights, n_evals = the sum of
 *              out_evals, n_rule_slots = the slots whose pg_slot_info rule index is >= 0,
 *              n_dead_rules = those of them with out_evals == 0 (0 when out_evals is not given)
 * The call is an audit, not traffic: it never touches the hit counters or their snapshots. Like
 * pg_reach_matrix it compiles and uploads stale tables first; it enqueues on hip_stream and
 * synchronises it, because the result comes back to the host. A zero n_src, n_dst or n_svc: PG_OK,
 * the given outputs cleared, *result zeroed apart from n_slots and layout_gen. PG_EINVAL
 * (pg_last_error says which): a null spec or result; both outputs null; a side above 2^20; more than
 * 4096 services; a weight above 65536; n_slots different from the current pg_num_counter_slots (the
 * ACLs changed since the caller sized its arrays); n_src * n_dst * sum of weights * 4 >= 2^63. */
typedef struct pg_reach_rules_spec {
    const uint32_t* src_ip;   /* the pg_reach_spec fields */
    size_t n_src;
    const uint32_t* dst_ip;
    size_t n_dst;
    const pg_service* services;
    size_t n_svc;
    const uint32_t* svc_weight; /* host, n_svc, or NULL */
    size_t n_slots;
} pg_reach_rules_spec;
typedef struct pg_reach_rules_result {   /* host */
    uint64_t layout_gen;
    uint64_t n_cells;
    uint64_t n_evals;
    uint32_t n_slots;
    uint32_t n_rule_slots;
    uint32_t n_dead_rules;
} pg_reach_rules_result;
int pg_reach_rules(pg_ctx* ctx, const pg_reach_rules_spec* spec, uint64_t* out_evals, uint64_t* out_cells,
                   pg_reach_rules_result* result, void* hip_stream);
/* TESTS ONLY -- never on the audit path: pg_reach_rules's per-word code, sink, windows and flushes
 * (rules.hpp, the templates the kernel instantiates and the plan the launch uses) run on the host,
 * work item by work item, with host output arrays. flags as in pg_debug_reach_matrix_host.
 * PG_EFAULT if a 32-bit window cell wrapped (the plan's flush bound rules that out). Does not touch
 * the device. */
int pg_debug_reach_rules_host(pg_ctx* ctx, const pg_reach_rules_spec* spec, uint64_t* out_evals, uint64_t* out_cells,
                              pg_reach_rules_result* result, int flags);
/* TESTS ONLY: the launch plan of a pg_reach_rules over n_slots slots, the last n_tail of them past
 * the rules, with the given outputs and a largest weight of max_weight under this context's
 * "rules_hist_cells", from the one function the launch itself uses (rules.hpp rules_plan): the
 * workgroup size; per histogram the LDS cells and the first index of its window (the window wraps
 * from the last index to index 0; cells_* in units of one 4 * s + c index); the words a workgroup may
 * process between two flushes; the LDS bytes. *resident (optional; needs the device) = the
 * workgroups the device holds at once under "blocks_per_cu". Launches nothing. */
typedef struct pg_reach_rules_plan {
    uint32_t block;
    uint32_t evals_cells, evals_base;
    uint32_t cells_cells, cells_base;
    uint32_t flush_words;
    uint32_t lds_bytes;
} pg_reach_rules_plan;
int pg_debug_reach_rules_plan(pg_ctx* ctx, uint32_t n_slots, uint32_t n_tail, int evals, int cells, uint32_t max_weight,
                              pg_reach_rules_plan* plan, uint32_t* resident);

/* ---- policy configurator ------------------------------------------
 * configurator.PolicyConfiguratorAPI / Txn (plugins/policy/configurator/configurator_api.go:28-54,
 * configurator_impl.go:104-472): K8s-shaped policies per pod -> ordered ContivRule lists
 * rendered into every registered renderer (the GPU ACL renderer and/or mock renderers).
 * The policy cache's pod data (LookupPod) and the IPAM NAT-loopback address are set
 * explicitly. Go nil-vs-empty matters for Match.Pods / IPBlocks: *_nil = 1 means nil. */
enum { PG_POLICY_INGRESS = 0, PG_POLICY_EGRESS = 1, PG_POLICY_ALL = 2 }; /* configurator.PolicyType */
enum { PG_MATCH_INGRESS = 0, PG_MATCH_EGRESS = 1 };                       /* configurator.MatchType  */
enum { PG_PORT_TCP = 0, PG_PORT_UDP = 1 };                                /* configurator.ProtocolType */
typedef struct pg_pod_id {
    const char* ns;
    const char* name;
} pg_pod_id;
typedef struct pg_cfg_port { /* configurator.Port */
    int32_t protocol;
    uint16_t number;
    uint16_t _pad;
} pg_cfg_port;
typedef struct pg_ipblock { /* configurator.IPBlock */
    pg_ipnet network;
    const pg_ipnet* except;
    size_t n_except;
} pg_ipblock;
typedef struct pg_match { /* configurator.Match */
    int32_t type;
    int32_t pods_nil;
    const pg_pod_id* pods;
    size_t n_pods;
    int32_t blocks_nil;
    int32_t _pad;
    const pg_ipblock* blocks;
    size_t n_blocks;
    const pg_cfg_port* ports;
    size_t n_ports;
} pg_match;
typedef struct pg_policy { /* configurator.ContivPolicy */
    pg_pod_id id;
    int32_t type;
    int32_t _pad;
    const pg_match* matches;
    size_t n_matches;
} pg_policy;

typedef struct pg_configurator pg_configurator;
typedef struct pg_cfg_txn pg_cfg_txn;
typedef struct pg_mock_renderer pg_mock_renderer;

pg_configurator* pg_configurator_new(void);
void pg_configurator_free(pg_configurator* c);
const char* pg_configurator_last_error(const pg_configurator* c);
/* PolicyConfigurator.RegisterRenderer (configurator_impl.go:104-107); the renderer must
 * outlive the configurator's transactions */
int pg_configurator_register_renderer(pg_configurator* c, pg_renderer* r);
int pg_configurator_register_mock(pg_configurator* c, pg_mock_renderer* r);
/* policy cache LookupPod data: ip = NULL removes the pod, "" = known without an address */
int pg_configurator_set_pod(pg_configurator* c, const char* ns, const char* name, const char* ip);
/* IPAM.NatLoopbackIP() (net.ParseIP form; NULL or unparsable = nil) */
int pg_configurator_set_nat_loopback(pg_configurator* c, const char* ip);
pg_cfg_txn* pg_configurator_new_txn(pg_configurator* c, int resync);
/* Txn.Configure: replaces the pod's set of policies (copied) */
int pg_cfg_txn_configure(pg_cfg_txn* t, const char* ns, const char* name, const pg_policy* policies, size_t n);
/* Txn.Commit: renders every configured pod into every renderer and commits them; frees t.
 * PG_EFAULT (message in pg_configurator_last_error) when a renderer's Commit failed. */
int pg_cfg_txn_commit(pg_cfg_txn* t);
void pg_cfg_txn_free(pg_cfg_txn* t);

/* mock/renderer.MockRenderer (mock/renderer/renderer_mock.go:39-185): stores the rendered
 * lists; TestTraffic evaluates them. direction: 0 = INGRESS (from the pod
 * to the vswitch), 1 = EGRESS; result: 0 DENIED, 1 ALLOWED, 2 UNMATCHED. */
pg_mock_renderer* pg_mock_renderer_new(void);
void pg_mock_renderer_free(pg_mock_renderer* r);
/* GetPodIP: writes the address ("" when unknown) and the mask length */
int pg_mock_renderer_pod_ip(pg_mock_renderer* r, const char* ns, const char* name, char* ip, size_t cap,
                            int* masklen);
/* the pod's ingress/egress list in rendered order -> number of rules (PG_ENOENT: no pod) */
int pg_mock_renderer_rules(pg_mock_renderer* r, const char* ns, const char* name, int direction,
                           pg_contiv_rule* out, size_t cap);
int pg_mock_renderer_test_traffic(pg_mock_renderer* r, const char* ns, const char* name, int direction,
                                  const char* src_ip, const char* dst_ip, int protocol, uint16_t src_port,
                                  uint16_t dst_port);
/* TestTraffic on the device: the pod's ingress (direction 0) / egress (1) list of r installed
 * in ctx as the ACL acl_name (a put, as by pg_apply_txn; again after a new Commit), so that
 * pg_classify(ctx, PG_MODE_SINGLE, pg_table_id(ctx, acl_name), ...) answers TestTraffic for
 * a batch: PERMIT = AllowedTraffic, DENY = DeniedTraffic (with the rule's slot), the ACL's
 * default slot = UnmatchedTraffic. Tuples carry the ContivRule protocol (TCP 0 / UDP 1 /
 * OTHER 2) and the destination port; TestTraffic's source-port test needs no field because
 * the configurator never sets a rule's source port -- a list that has one (or a protocol-OTHER
 * rule) is refused with PG_EINVAL. PG_ENOENT: the pod was not rendered (TestTraffic:
 * UnmatchedTraffic for every packet). */
int pg_mock_renderer_install(pg_ctx* ctx, const pg_mock_renderer* r, const char* ns, const char* name, int direction,
                             const char* acl_name);

/* ---- K8s policy cache and processor ------------------------------
 * The KSR objects cross the boundary in their protobuf wire form (proto.Marshal of
 * plugins/ksr/model/{pod,namespace,policy}.Pod / Namespace / Policy), so the Go side
 * passes what it holds. policy.Policy_LabelSelector travels the same way for queries.
 * cache.PolicyCacheAPI (plugins/policy/cache/cache_api.go:30-116, cache_impl.go),
 * processor.PolicyProcessor (plugins/policy/processor/processor.go:34-527). Name lists come
 * back sorted and '\n'-joined (the reference returns them in Go map order). */
typedef struct pg_policy_cache pg_policy_cache;
typedef struct pg_policy_processor pg_policy_processor;
enum { PG_K8S_POD = 0, PG_K8S_NAMESPACE = 1, PG_K8S_POLICY = 2 };
enum {
    PG_Q_PODS_BY_LABEL_SELECTOR_INSIDE_NS = 0, /* arg = namespace, selector        */
    PG_Q_PODS_BY_NS_LABEL_SELECTOR = 1,        /* selector                         */
    PG_Q_PODS_BY_NAMESPACE = 2,                /* arg = namespace                  */
    PG_Q_ALL_PODS = 3,
    PG_Q_POLICIES_BY_POD = 4,                  /* arg = "ns/name"                  */
    PG_Q_ALL_POLICIES = 5,
    PG_Q_ALL_NAMESPACES = 6,
    PG_Q_MATCH_LABEL_PODS_INSIDE_NS = 7,       /* arg = namespace, selector labels (match_label.go) */
    PG_Q_PODS_BY_NS_LABELS = 8,                /* selector labels                  */
    PG_Q_MATCH_EXPRESSION_PODS_INSIDE_NS = 9,  /* arg = namespace, selector expressions (match_expression.go) */
    PG_Q_PODS_BY_NS_EXPRESSIONS = 10,          /* selector expressions             */
    /* secondary indexes (podmap.go / namespacemap.go / policymap.go), arg = index value */
    PG_Q_IDX_POD_LABEL = 11, PG_Q_IDX_POD_KEY = 12, PG_Q_IDX_POD_NS_LABEL = 13, PG_Q_IDX_POD_NS_KEY = 14,
    PG_Q_IDX_NS_LABEL = 15, PG_Q_IDX_NS_KEY = 16, PG_Q_IDX_POLICY_LABEL = 17, PG_Q_IDX_POLICY_NS_LABEL = 18
};
pg_policy_cache* pg_policy_cache_new(void);
void pg_policy_cache_free(pg_policy_cache* c);
const char* pg_policy_cache_last_error(const pg_policy_cache* c);
/* ConfigIndex.Register* / Unregister* (index only, no events); pb NULL = a nil object.
 * unregister -> 1 found, 0 not */
int pg_policy_cache_register(pg_policy_cache* c, int kind, const char* id, const uint8_t* pb, size_t len);
int pg_policy_cache_unregister(pg_policy_cache* c, int kind, const char* id);
/* Update (data_change.go): prev NULL = add, next NULL = delete, both = update; the
 * watchers (processor) run inside. PG_EFAULT + last_error when a watcher fails. */
int pg_policy_cache_update(pg_policy_cache* c, int kind, const uint8_t* prev, size_t prev_len, const uint8_t* next,
                           size_t next_len);
/* Resync (data_resync.go): the whole K8s state, n objects of the given kinds */
int pg_policy_cache_resync(pg_policy_cache* c, const int* kinds, const uint8_t* const* objs, const size_t* lens,
                           size_t n);
/* Lookup{Pod,Namespace,Policy}: 1 found (wire bytes as registered -> out, *out_len; a nil
 * object has *out_len = (size_t)-1), 0 not found */
int pg_policy_cache_lookup(const pg_policy_cache* c, int kind, const char* id, uint8_t* out, size_t cap,
                           size_t* out_len);
/* name-list queries -> number of names; '\n'-joined into out when *out_len (bytes, no NUL)
 * fits cap */
int pg_policy_cache_query(const pg_policy_cache* c, int query, const char* arg, const uint8_t* selector,
                          size_t selector_len, char* out, size_t cap, size_t* out_len);
/* PolicyProcessor watching the cache and configuring cfg (which then looks pods up in the
 * cache); pod_subnet = IPAM.PodSubnetThisNode() */
pg_policy_processor* pg_policy_processor_new(pg_policy_cache* c, pg_configurator* cfg, const pg_ipnet* pod_subnet);
void pg_policy_processor_free(pg_policy_processor* p);
/* Process(resync, pods) with pods as "ns/name" */
int pg_policy_processor_process(pg_policy_processor* p, int resync, const char* const* pods, size_t n);
const char* pg_policy_processor_last_error(const pg_policy_processor* p);

/* ---- VPPTCP renderer and VPP session-rule tables -------------------
 * The renderer cache's second consumer: IngressOrientation tables rendered as VPP session
 * rules for the VPP TCP host stack.
 *   vpptcp.Renderer Init/NewTxn/Render/Commit  plugins/policy/renderer/vpptcp/vpptcp_renderer.go:58-188
 *   dumpRules / updateRules                    vpptcp_renderer.go:191-316
 *   rule.SessionRule, Export/ImportSessionRules plugins/policy/renderer/vpptcp/rule/session_rule.go:72-476
 *   rule.IPv4Net (GetNsIndex/GetPodByAppNsIndex) session_rule.go:88-95      -> pg_appns
 *   session_rule_add_del / session_rules_dump  binary API as mock/sessionrules/sessionrules_mock.go
 *                                              holds it                    -> pg_session_rules
 * Host-side control plane: the reference classifies nothing on this path (the session-rule
 * lookup is VPP's). */
enum { PG_SCOPE_GLOBAL = 1, PG_SCOPE_LOCAL = 2, PG_SCOPE_BOTH = 3 };
#define PG_SR_ACTION_DO_NOTHING 0xFFFFFFFFu
#define PG_SR_ACTION_DENY 0xFFFFFFFEu
#define PG_SR_ACTION_ALLOW 0xFFFFFFFDu
typedef struct pg_session_rule { /* rule.SessionRule (session_rule.go:73-86) */
    uint8_t transport_proto;     /* 0 TCP, 1 UDP */
    uint8_t is_ip4;
    uint8_t lcl_ip[16];
    uint8_t lcl_plen;
    uint8_t rmt_ip[16];
    uint8_t rmt_plen;
    uint16_t lcl_port;
    uint16_t rmt_port;
    uint32_t action_index;
    uint32_t appns_index;
    uint8_t scope;
    char tag[64];
} pg_session_rule;
typedef struct pg_session_rules pg_session_rules;
typedef struct pg_appns pg_appns;
typedef struct pg_vpptcp_renderer pg_vpptcp_renderer;
typedef struct pg_vpptcp_txn pg_vpptcp_txn;

/* VPP's session-rule tables; tag_prefix NULL = "contiv/vpp-policy" (rules with another tag
 * are refused). Every add/del counts one request, a dump two (dump + control_ping). */
pg_session_rules* pg_session_rules_new(const char* tag_prefix);
void pg_session_rules_free(pg_session_rules* s);
int pg_session_rules_clear(pg_session_rules* s);
int pg_session_rules_counts(const pg_session_rules* s, int* req_count, int* err_count);
/* session_rule_add_del: the reply's retval (0 ok, 1 refused: bad tag, duplicate add, unknown delete) */
int pg_session_rule_add_del(pg_session_rules* s, const pg_session_rule* rule, int is_add);
/* rules of the global table (scope GLOBAL) or of ns_index's local table (scope LOCAL), in
 * installation order -> count (copies min(count, cap)) */
int pg_session_rules_table(const pg_session_rules* s, int scope, uint32_t ns_index, pg_session_rule* out, size_t cap);
/* MockSessionRules.{Local,Global}Table().HasRule: "" = unset address, a bare address = its
 * one-host subnet; proto "TCP"/"UDP"; action "ALLOW"/"DENY" -> 1 / 0 */
int pg_session_rules_has_rule(const pg_session_rules* s, int scope, uint32_t ns_index, const char* lcl_ip,
                              uint16_t lcl_port, const char* rmt_ip, uint16_t rmt_port, const char* proto,
                              const char* action);
/* pod -> VPP application namespace index (IPv4Net.GetNsIndex / GetPodByAppNsIndex) */
pg_appns* pg_appns_new(void);
void pg_appns_free(pg_appns* a);
int pg_appns_set(pg_appns* a, const char* pod_namespace, const char* pod_name, uint32_t ns_index);
/* ExportSessionRules: pod_name NULL = global table -> count (copies min(count, cap)) */
int pg_export_session_rules(const pg_appns* a, const pg_contiv_rule* rules, size_t n, const char* pod_namespace,
                            const char* pod_name, const pg_ipnet* pod_ip, pg_session_rule* out, size_t cap);
/* the renderer keeps pointers to vpp and ipv4net (both must outlive it); chan_buf_size =
 * GoVPPChanBufSize (0 = 100: requests are sent in bursts of that size) */
pg_vpptcp_renderer* pg_vpptcp_renderer_new(pg_session_rules* vpp, const pg_appns* ipv4net, int chan_buf_size);
void pg_vpptcp_renderer_free(pg_vpptcp_renderer* r);
const char* pg_vpptcp_last_error(const pg_vpptcp_renderer* r);
pg_vpptcp_txn* pg_vpptcp_new_txn(pg_vpptcp_renderer* r, int resync);
int pg_vpptcp_txn_render(pg_vpptcp_txn* t, const char* pod_namespace, const char* pod_name, const pg_ipnet* pod_ip,
                         const pg_contiv_rule* ingress, size_t n_ingress, const pg_contiv_rule* egress,
                         size_t n_egress, int removed);
/* renders and programs the session rules, frees t; PG_EFAULT + pg_vpptcp_last_error when a
 * request failed (the cache then keeps its previous state, as the reference's does) */
int pg_vpptcp_txn_commit(pg_vpptcp_txn* t);
void pg_vpptcp_txn_free(pg_vpptcp_txn* t);
/* PolicyConfigurator.RegisterRenderer for the VPPTCP renderer */
int pg_configurator_register_vpptcp(pg_configurator* c, pg_vpptcp_renderer* r);

/* VPP's session-rule lookup on the device. Installs the session-rule table (scope PG's
 * kScopeLocal = 2 with its application-namespace index, or kScopeGlobal = 1) of s into ctx as
 * the ACL acl_name (a put, as by pg_apply_txn; call again after the table changed), so that
 * pg_classify(ctx, PG_MODE_SINGLE, pg_table_id(ctx, acl_name), ...) classifies connections by
 * it: the table's IPv4 rules (prefixes up to 32 bits) ordered most specific first (lcl_plen + rmt_plen + one per set
 * port, ties in SessionRule.Compare order, session_rule.go:168-209) and first match, which is
 * the containment order renderer/api.go:111-112 defines for the ContivRules they come from
 * (convertContivRule, session_rule.go:263-361). Tuple fields: a local table keys on
 * (src_ip = local address, dst_ip = remote address, dst_port = remote port), the global table
 * on (src_ip = remote, dst_ip = local, dst_port = local port); proto TCP / UDP. Verdict PERMIT =
 * ALLOW, DENY = DENY with the rule's slot, the ACL's default slot = no session rule applies.
 * The reference has no session-rule lookup (VPP's own code): parity unpinned beyond the
 * restatement in oracle/vpptcp.py. PG_EINVAL (+ pg_last_error) for a rule this form cannot
 * hold: a port on the side the table does not key on, an action other than ALLOW / DENY. */
int pg_session_table_install(pg_ctx* ctx, const pg_session_rules* s, int scope, uint32_t ns_index,
                             const char* acl_name);

#ifdef __cplusplus
}
#endif
#endif /* POLICYGPU_H */
