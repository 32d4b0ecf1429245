"""Python mirror of Shadow's topology interface (src/topology/shd-topology.h:14-22) over the
MI355X engine in libshdtopo.so.

Method names, argument meaning and error behaviour follow the reference:

* ``Topology.new(path)``            topology_new            (shd-topology.c:1237) -- None on failure
* ``attach(address, random, ...)``  topology_attach         (shd-topology.c:1154) -- one
                                    random_nextDouble draw on the host stream unless LPM
* ``detach(address)``               topology_detach         (shd-topology.c:1190)
* ``getLatency / getReliability``   (shd-topology.c:940-958) -- -1.0 for an unattached address
* ``isRoutable``                    (shd-topology.c:960)
* ``getMinimumLatency``             new: global min over attached pairs
* ``routePacketBatch``              new: worker_schedulePacket for a window (shd-worker.c:332-370)

``Address`` / ``Random`` are the shim restatements of Shadow's objects (libshdtopo_shim.so) so
that the exact C entry points are exercised.  Every computation runs in the HIP library; this
module only marshals arguments.
"""
from __future__ import annotations

import ctypes
import socket
import struct

import numpy as np

from . import _lib as L


def ip_to_network(ip: str) -> int:
    """dotted quad -> in_addr_t as Shadow holds it (network byte order in memory)."""
    return struct.unpack("<I", socket.inet_aton(ip))[0]


def network_to_ip(n: int) -> str:
    return socket.inet_ntoa(struct.pack("<I", n & 0xFFFFFFFF))


class Address:
    """Shadow Address (shd-address.c): only the network-order IP is used by the topology."""

    def __init__(self, ip):
        lib, shim = L.load()
        self.ip = ip_to_network(ip) if isinstance(ip, str) else int(ip)
        self._p = shim.shim_address_new(self.ip)
        self._shim = shim

    def __del__(self):
        try:
            self._shim.shim_address_free(self._p)
        except Exception:
            pass


class Random:
    """Shadow Random (shd-random.c): glibc rand_r stream."""

    def __init__(self, seed: int):
        lib, shim = L.load()
        self._p = shim.random_new(seed & 0xFFFFFFFF)
        self._shim = shim

    @property
    def state(self) -> int:
        return int(self._shim.shim_random_state(self._p))

    def nextDouble(self) -> float:
        return float(self._shim.random_nextDouble(self._p))

    def nextInt(self) -> int:
        return int(self._shim.random_nextInt(self._p))

    def __del__(self):
        try:
            self._shim.random_free(self._p)
        except Exception:
            pass


# one record of Topology.link_crossings (ShdCrossing)
CROSSING_DTYPE = np.dtype([("flow", np.int32), ("watch", np.int32), ("hop", np.int32),
                           ("reverse", np.int32)])


# one record of Topology.table_diff (ShdTableChange)
TABLE_CHANGE_DTYPE = np.dtype([("srcCol", np.int32), ("dstCol", np.int32), ("lat0", np.float64),
                               ("lat1", np.float64), ("rel0", np.float64), ("rel1", np.float64),
                               ("hops0", np.uint16), ("hops1", np.uint16), ("kind", np.uint32)])


# one record of Topology.flow_impact (ShdFlowChange)
FLOW_CHANGE_DTYPE = np.dtype([("flow", np.int64), ("lat0", np.float64), ("lat1", np.float64),
                              ("rel0", np.float64), ("rel1", np.float64), ("hops0", np.uint16),
                              ("hops1", np.uint16), ("kind", np.uint32)])


# one record of Topology.load_shift (ShdLoadChange)
LOAD_CHANGE_DTYPE = np.dtype([("kind", np.int32), ("id", np.int32), ("idA", np.int32),
                              ("idB", np.int32), ("before", np.uint64), ("after", np.uint64)])


def crossings_by_watch(result):
    """Invert a Topology.link_crossings result into {watch index: flow indices} -- every watch of
    the call, the flows ascending, a flow once per record (host side: the records are already in
    flow order, so a stable sort by watch is enough)."""
    rec = result["records"]
    order = np.argsort(rec["watch"], kind="stable")
    watch, flow = rec["watch"][order], rec["flow"][order]
    nw = len(result["count"])
    cut = np.searchsorted(watch, np.arange(nw + 1))
    return {k: flow[cut[k]:cut[k + 1]].copy() for k in range(nw)}


def _b(s):
    return None if s is None else s.encode()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Topology:
    def __init__(self, handle):
        self._lib, self._shim = L.load()
        self._h = handle

    # ---- construction ----
    @classmethod
    def new(cls, graph_path: str):
        lib, _ = L.load()
        h = lib.topology_new(graph_path.encode())
        return cls(h) if h else None

    @classmethod
    def from_buffer(cls, graphml: bytes):
        lib, _ = L.load()
        h = lib.shdtopo_new_from_buffer(graphml, len(graphml))
        return cls(h) if h else None

    @classmethod
    def synthetic(cls, seed=20261015, n_routers=990_000, n_poi=10_000, n_edges=10_000_000,
                  integer_latency=False, alpha=1.0 / 1.1, directed=False):
        lib, _ = L.load()
        p = L.ShdSynthParams(seed, n_routers, n_poi, n_edges, int(integer_latency), alpha,
                             int(directed))
        h = lib.shdtopo_new_synthetic(ctypes.byref(p))
        return cls(h) if h else None

    def free(self):
        if self._h:
            self._lib.topology_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def set_option(self, key: str, value: float):
        if self._lib.shdtopo_set_option(self._h, key.encode(), float(value)) != 0:
            raise KeyError(key)

    # ---- reference API ----
    def attach(self, address: Address, random: Random, ipHint=None, geocodeHint=None,
               typeHint=None):
        down = ctypes.c_uint64(0)
        up = ctypes.c_uint64(0)
        self._lib.topology_attach(self._h, address._p, random._p, _b(ipHint), _b(geocodeHint),
                                  _b(typeHint), ctypes.byref(down), ctypes.byref(up))
        return down.value, up.value

    def detach(self, address: Address):
        self._lib.topology_detach(self._h, address._p)

    def isRoutable(self, src: Address, dst: Address) -> bool:
        return bool(self._lib.topology_isRoutable(self._h, src._p, dst._p))

    def getLatency(self, src: Address, dst: Address) -> float:
        return self._lib.topology_getLatency(self._h, src._p, dst._p)

    def getReliability(self, src: Address, dst: Address) -> float:
        return self._lib.topology_getReliability(self._h, src._p, dst._p)

    def getMinimumLatency(self) -> float:
        return self._lib.topology_getMinimumLatency(self._h)

    def lazyMinimumLatency(self) -> float:
        return self._lib.shdtopo_get_lazy_minimum_latency(self._h)

    def routePacketBatch(self, src_ip, dst_ip, payload, rng_state, now, jump_ns, clamp=True):
        n = len(src_ip)
        ins = (L.TopoPacketIn * n)()
        for i in range(n):
            ins[i].srcIP = int(src_ip[i])
            ins[i].dstIP = int(dst_ip[i])
            ins[i].payloadLength = int(payload[i])
            ins[i].rngState = int(rng_state[i])
            ins[i].now = int(now[i])
        outs = (L.TopoPacketOut * n)()
        r = self._lib.topology_routePacketBatch(self._h, ins, outs, n, int(jump_ns), int(clamp))
        if r < 0:
            raise RuntimeError("topology_routePacketBatch failed: %d" % r)
        self.last_unrouted = r  # packets whose address is not attached (delivered 0)
        t = np.array([o.time for o in outs], dtype=np.uint64)
        st = np.array([o.rngState for o in outs], dtype=np.uint32)
        dl = np.array([o.delivered for o in outs], dtype=np.uint8)
        return t, dl, st

    # ---- raw-IP helpers ----
    def attach_ip(self, ip, state, ipHint=None, geocodeHint=None, typeHint=None):
        st = ctypes.c_uint32(state & 0xFFFFFFFF)
        v = self._lib.shdtopo_attach_ip(self._h, int(ip), ctypes.byref(st), _b(ipHint),
                                        _b(geocodeHint), _b(typeHint), None, None)
        return v, st.value

    def detach_ip(self, ip):
        self._lib.shdtopo_detach_ip(self._h, int(ip))

    def latency_ip(self, s, d):
        return self._lib.shdtopo_get_latency_ip(self._h, int(s), int(d))

    def reliability_ip(self, s, d):
        return self._lib.shdtopo_get_reliability_ip(self._h, int(s), int(d))

    # ---- graph / table ----
    @property
    def num_vertices(self):
        return int(self._lib.shdtopo_num_vertices(self._h))

    @property
    def num_edges(self):
        return int(self._lib.shdtopo_num_edges(self._h))

    @property
    def is_complete(self):
        return bool(self._lib.shdtopo_is_complete(self._h))

    @property
    def is_directed(self):
        return bool(self._lib.shdtopo_is_directed(self._h))

    def attached_vertices(self):
        n = int(self._lib.shdtopo_num_attached(self._h))
        out = np.empty(max(n, 1), np.int32)
        self._lib.shdtopo_attached_vertices(self._h, _p(out), n)
        return out[:n]

    def vertex_of_ip(self, ip):
        return int(self._lib.shdtopo_vertex_of_ip(self._h, int(ip)))

    def lazy_rows(self):
        """Test hook (shdtopo_lazy_rows): the materialised source rows -- (vertices, epochs, the
        row minimum each latest materialisation offered to the running minimum)."""
        n = int(self._lib.shdtopo_lazy_rows(self._h, None, None, None, 0))
        v = np.empty(max(n, 1), np.int32)
        e = np.empty(max(n, 1), np.uint64)
        m = np.empty(max(n, 1), np.float64)
        n = int(self._lib.shdtopo_lazy_rows(self._h, _p(v), _p(e), _p(m), n))
        return v[:n], e[:n], m[:n]

    def column_of_ip(self, ip):
        return int(self._lib.shdtopo_column_of_ip(self._h, int(ip)))

    def build(self):
        r = self._lib.shdtopo_build(self._h)
        if r != 0:
            raise RuntimeError("shdtopo_build failed: %d" % r)

    def table(self):
        """Host copy of the A x A table: (attached vertices, lat, rel, hops)."""
        self.build()
        a = self.attached_vertices()
        n = len(a)
        lat = np.empty((n, n), np.float64)
        rel = np.empty((n, n), np.float64)
        hops = np.empty((n, n), np.uint16)
        r = self._lib.shdtopo_table_to_host(self._h, _p(lat), _p(rel), _p(hops))
        if r != 0:
            raise RuntimeError("shdtopo_table_to_host failed: %d" % r)
        return a, lat, rel, hops

    def stats(self):
        s = L.ShdStats()
        r = self._lib.shdtopo_get_stats(self._h, ctypes.byref(s))
        if r != 0:
            raise RuntimeError("shdtopo_get_stats failed: %d" % r)
        out = {k: getattr(s, k) for k, _ in L.ShdStats._fields_}
        out["phase_ms"] = list(out["phase_ms"])
        out["parent_phase_ms"] = list(out["parent_phase_ms"])
        out["replay_lines"] = list(out["replay_lines"])
        out["replay_phase_ms"] = list(out["replay_phase_ms"])
        out["replay_sink_ms"] = list(out["replay_sink_ms"])
        out["batch_wave_ms"] = list(out["batch_wave_ms"])
        out["csr_step_ms"] = list(out["csr_step_ms"])
        out["build_step_ms"] = list(out["build_step_ms"])
        out["walk_kinds"] = list(out["walk_kinds"])
        for k in ("device_kernel_ms", "device_build_ms", "device_rows", "attach_prep_step_ms",
                  "sweep_events", "write_lines", "read_lines"):
            out[k] = list(out[k])
        out["events"] = dict(zip(("expanded", "tail_relax", "tail_improve", "window_taken",
                                  "overflow_refilled", "parent_vertices", "tail_settled_relax",
                                  "stale_skipped"),
                                 list(out["events"])))
        return out

    def export_graph(self):
        """(V, eu, ev, elat, eloss, vloss) host arrays of the parsed graph (document order)."""
        V, E = self.num_vertices, self.num_edges
        eu = np.empty(E, np.int32)
        ev = np.empty(E, np.int32)
        el = np.empty(E, np.float64)
        lo = np.empty(E, np.float64)
        vl = np.empty(V, np.float64)
        if self._lib.shdtopo_export_graph(self._h, _p(eu), _p(ev), _p(el), _p(lo), _p(vl)) != 0:
            raise RuntimeError("export_graph failed")
        return V, eu, ev, el, lo, vl

    def export_csr(self):
        """Test hook (shdtopo_export_csr): the GPU-prepared CSR -- perm (new -> old), rowptr, the
        adjacency columns, pi = d(h0, .) and the h0-tree parents, relabelled ids."""
        n = int(self._lib.shdtopo_export_csr(self._h, None, None, None, None, None))
        if n < 0:
            raise RuntimeError("shdtopo_export_csr failed: %d" % n)
        V = self.num_vertices
        perm = np.empty(V, np.int32)
        rowptr = np.empty(V + 1, np.uint32)
        col = np.empty(max(n, 1), np.uint32)
        pot = np.empty(V, np.float64)
        par = np.empty(V, np.uint32)
        r = self._lib.shdtopo_export_csr(self._h, _p(perm), _p(rowptr), _p(col), _p(pot), _p(par))
        if r != n:
            raise RuntimeError("shdtopo_export_csr failed: %d" % r)
        return dict(perm=perm, rowptr=rowptr, col=col[:n], pot=pot, tree_parent=par)

    # name -> (dtype, trailing shape) of shdtopo_export_prep's arrays
    PREP_ARRAYS = {
        "perm": (np.int32, ()), "inv": (np.int32, ()), "rowptr": (np.uint32, ()),
        "adj": (np.uint32, (4,)), "aloss": (np.float64, ()), "vloss": (np.float64, ()),
        "self_lat": (np.float64, ()), "self_loss": (np.float64, ()), "pot": (np.float64, ()),
        "pi_max": (np.float64, ()), "spt_parent": (np.uint32, ()), "spt": (np.uint32, (8,)),
        "adjk": (np.uint32, (4,)), "kap": (np.float32, ()), "ksum": (np.float32, None),
        "kap0": (np.float32, ()), "kf_kap": (np.float64, ()), "hub_seg": (np.uint32, (2,)),
        "hub_multi": (np.uint32, (4,)), "rowptr_in": (np.uint32, ()),
        "adj_out": (np.uint32, (4,)), "pot_src": (np.float64, ()), "tbits": (np.uint32, ()),
        "tbits_eff": (np.uint32, ()), "dead": (np.uint32, ()), "tleaf": (np.uint32, (8,)),
        "kfix": (np.float64, ()), "state": (np.int32, ()),
    }
    PREP_STATE = ("adjk_plain", "flagged", "resorted", "leaf", "kprobes", "kap_in_rec",
                  "hub_seg_len", "group_hubs")

    def export_prep(self, names=None):
        """Test hook (shdtopo_export_prep): the prepared arrays by name, relabelled ids -- every
        array that exists in the topology's current state when names is None (an array that does
        not: KeyError when asked for by name).  ``state`` comes back as a dict, ``ksum`` as
        [V, probes]."""
        out = {}
        for name in (names if names is not None else self.PREP_ARRAYS):
            dt, shape = self.PREP_ARRAYS[name]
            n = int(self._lib.shdtopo_export_prep(self._h, name.encode(), None, 0))
            if n == -2 and names is None:
                continue
            if n == -2:
                raise KeyError(name)
            if n < 0:
                raise RuntimeError("shdtopo_export_prep(%s) failed: %d" % (name, n))
            buf = np.empty(max(n, 1), np.uint8)
            r = int(self._lib.shdtopo_export_prep(self._h, name.encode(), _p(buf), n))
            if r != n:
                raise RuntimeError("shdtopo_export_prep(%s) failed: %d" % (name, r))
            out[name] = buf[:n].view(dt)
        if "state" in out:
            out["state"] = dict(zip(self.PREP_STATE, (int(x) for x in out["state"])))
        for name, a in out.items():
            if name == "state":
                continue
            shape = self.PREP_ARRAYS[name][1]
            if shape is None:  # ksum: one row of probes per vertex
                a = a.reshape(self.num_vertices, -1)
            elif shape:
                a = a.reshape((-1,) + shape)
            out[name] = a
        return out

    def replay_source(self, src, full=True):
        """Test hook (shdtopo_replay_source): the exact heap replay's (dist, parent vertex) from
        vertex `src`, original ids; full=False stops when every attached vertex is popped."""
        V = self.num_vertices
        dist = np.empty(V, np.float64)
        par = np.empty(V, np.int32)
        r = self._lib.shdtopo_replay_source(self._h, int(src), int(bool(full)), _p(dist), _p(par))
        if r != 0:
            raise RuntimeError("shdtopo_replay_source failed: %d" % r)
        return dist, par

    # ---- route tracing ----
    def trace_routes(self, src_ips, dst_ips, cap=None):
        """shdtopo_trace_routes: the vertex / edge route of every (src, dst) host pair, the
        forward route of the source's table row.  Returns a dict of numpy arrays: per request
        ``offset, hops, status, latency, reliability`` and the concatenated ``vertices, edges``
        (route i = entries [offset, offset + hops]; edges[offset + hops] = -1), plus ``total``,
        the entries every route needs.  cap=None sizes the buffers first (a cap = 0 call); a
        smaller cap writes only the routes that fit (the others: status 3, offset -1)."""
        s = np.ascontiguousarray(src_ips, dtype=np.uint32)
        d = np.ascontiguousarray(dst_ips, dtype=np.uint32)
        if s.shape != d.shape or s.ndim != 1:
            raise ValueError("src_ips and dst_ips must be 1-D and of one length")
        n = len(s)
        routes = (L.ShdRoute * max(n, 1))()
        if cap is None:
            cap = int(self._lib.shdtopo_trace_routes(self._h, _p(s), _p(d), n, routes, None,
                                                     None, 0))
            if cap < 0:
                raise RuntimeError("shdtopo_trace_routes failed: %d" % cap)
        cap = int(cap)
        vertices = np.full(max(cap, 1), -2, np.int32)
        edges = np.full(max(cap, 1), -2, np.int32)
        total = int(self._lib.shdtopo_trace_routes(self._h, _p(s), _p(d), n, routes,
                                                   _p(vertices) if cap else None,
                                                   _p(edges) if cap else None, cap))
        if total < 0:
            raise RuntimeError("shdtopo_trace_routes failed: %d" % total)
        r = np.frombuffer(routes, dtype=np.dtype(
            [("offset", np.int64), ("hops", np.int32), ("status", np.int32),
             ("latency", np.float64), ("reliability", np.float64)]), count=n)
        out = {k: r[k].copy() for k in ("offset", "hops", "status", "latency", "reliability")}
        out["vertices"] = vertices[:cap]
        out["edges"] = edges[:cap]
        out["total"] = total
        return out

    def format_route(self, trace, i):
        """shdtopo_format_route: the reference's debug line (shd-topology.c:654-656, the text after
        ``debug(``) for request i of a trace_routes result."""
        r = L.ShdRoute(int(trace["offset"][i]), int(trace["hops"][i]), int(trace["status"][i]),
                       float(trace["latency"][i]), float(trace["reliability"][i]))
        v = np.ascontiguousarray(trace["vertices"], dtype=np.int32)
        e = np.ascontiguousarray(trace["edges"], dtype=np.int32)
        n = int(self._lib.shdtopo_format_route(self._h, ctypes.byref(r), _p(v), _p(e), None, 0))
        if n < 0:
            raise RuntimeError("shdtopo_format_route failed: %d" % n)
        buf = ctypes.create_string_buffer(n + 1)
        self._lib.shdtopo_format_route(self._h, ctypes.byref(r), _p(v), _p(e), buf, n + 1)
        return buf.value.decode()

    def trace_stats(self):
        """The last trace's own counters (shdtopo_trace_stats)."""
        s = L.ShdTraceStats()
        if self._lib.shdtopo_trace_stats(self._h, ctypes.byref(s)) != 0:
            raise RuntimeError("shdtopo_trace_stats failed")
        return {k: getattr(s, k) for k, _ in L.ShdTraceStats._fields_}

    # ---- link load ----
    def link_load(self, src_ips, dst_ips, weight=None):
        """shdtopo_link_load: the weight the flows (src, dst, weight) put on every edge and
        vertex along the routes trace_routes reports.  weight=None counts 1 per flow.  Returns a
        dict of numpy uint64 arrays -- ``edge_fwd[e]`` (hops leaving eu[e]; self loops; every arc
        of a directed topology), ``edge_rev[e]`` (hops leaving ev[e]), ``vertex[v]`` (the weight
        arriving at v, original ids) -- and ``routed``, the flows that contributed."""
        s = np.ascontiguousarray(src_ips, dtype=np.uint32)
        d = np.ascontiguousarray(dst_ips, dtype=np.uint32)
        if s.shape != d.shape or s.ndim != 1:
            raise ValueError("src_ips and dst_ips must be 1-D and of one length")
        n = len(s)
        w = None
        if weight is not None:
            w = np.ascontiguousarray(weight, dtype=np.uint64)
            if w.shape != s.shape:
                raise ValueError("weight must have one entry per flow")
        E, V = self.num_edges, self.num_vertices
        edge = np.zeros(max(2 * E, 1), np.uint64)
        vert = np.zeros(max(V, 1), np.uint64)
        r = int(self._lib.shdtopo_link_load(self._h, _p(s), _p(d), _p(w) if w is not None else None,
                                            n, _p(edge), _p(vert)))
        if r < 0:
            raise RuntimeError("shdtopo_link_load failed: %d" % r)
        return {"edge_fwd": edge[:E], "edge_rev": edge[E:2 * E], "vertex": vert[:V], "routed": r}

    def link_load_stats(self):
        """The last link_load's own counters (shdtopo_link_load_stats)."""
        s = L.ShdLoadStats()
        if self._lib.shdtopo_link_load_stats(self._h, ctypes.byref(s)) != 0:
            raise RuntimeError("shdtopo_link_load_stats failed")
        return {k: getattr(s, k) for k, _ in L.ShdLoadStats._fields_}

    # ---- link crossings ----
    def link_crossings(self, src_ips, dst_ips, edges=(), vertices=(), weight=None, cap=None):
        """shdtopo_link_crossings: the hops of the flows (src, dst, weight) that go over a watched
        edge (``edges``: edge ids) or arrive at a watched vertex (``vertices``: vertex ids), along
        the routes trace_routes reports.  Returns a dict: ``total``, the number of crossings;
        ``offsets`` int64[n + 1], the running sum of the flows' record counts; ``records``, a
        structured array (CROSSING_DTYPE: flow, watch, hop, reverse) ordered by flow, hop, edge
        before vertex -- watch k < len(edges) is edges[k], len(edges) + k is vertices[k]; and per
        watch ``count`` (its records) and ``weight`` (their flows' summed weight), uint64.
        cap=None sizes the buffer first (a cap = 0 call); a smaller cap writes only the flows
        whose records end at or below it (``records`` then has offsets[i + 1] <= cap entries)."""
        s = np.ascontiguousarray(src_ips, dtype=np.uint32)
        d = np.ascontiguousarray(dst_ips, dtype=np.uint32)
        if s.shape != d.shape or s.ndim != 1:
            raise ValueError("src_ips and dst_ips must be 1-D and of one length")
        n = len(s)
        w = None
        if weight is not None:
            w = np.ascontiguousarray(weight, dtype=np.uint64)
            if w.shape != s.shape:
                raise ValueError("weight must have one entry per flow")
        we = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1)
        wv = np.ascontiguousarray(vertices, dtype=np.int32).reshape(-1)
        nw = len(we) + len(wv)
        offsets = np.zeros(n + 1, np.int64)
        count = np.zeros(max(nw, 1), np.uint64)
        wsum = np.zeros(max(nw, 1), np.uint64)

        def call(out, c):
            return int(self._lib.shdtopo_link_crossings(
                self._h, _p(s), _p(d), _p(w) if w is not None else None, n,
                _p(we) if len(we) else None, len(we), _p(wv) if len(wv) else None, len(wv),
                _p(offsets), _p(out) if c else None, c, _p(count), _p(wsum)))
        if cap is None:
            cap = call(None, 0)
            if cap < 0:
                raise RuntimeError("shdtopo_link_crossings failed: %d" % cap)
        cap = int(cap)
        records = np.zeros(max(cap, 1), CROSSING_DTYPE)
        total = call(records, cap)
        if total < 0:
            raise RuntimeError("shdtopo_link_crossings failed: %d" % total)
        fit = int(offsets[np.searchsorted(offsets, cap, side="right") - 1]) if cap else 0
        return {"total": total, "offsets": offsets, "records": records[:fit],
                "count": count[:nw], "weight": wsum[:nw]}

    def link_crossings_stats(self):
        """The last link_crossings' own counters (shdtopo_link_crossings_stats)."""
        s = L.ShdCrossStats()
        if self._lib.shdtopo_link_crossings_stats(self._h, ctypes.byref(s)) != 0:
            raise RuntimeError("shdtopo_link_crossings_stats failed")
        return {k: getattr(s, k) for k, _ in L.ShdCrossStats._fields_}

    # ---- link timeline ----
    def link_timeline(self, src_ips, dst_ips, now=None, edges=(), vertices=(), weight=None, t0=0,
                      bin_ns=1_000_000, nbins=0):
        """shdtopo_link_timeline: the weight of the flows (src, dst, weight) per time bin on the
        watched edges (``edges``: edge ids) and vertices (``vertices``: vertex ids), along the
        routes trace_routes reports.  ``now`` is each flow's emission time in ns (None: 0 each,
        the bins are then time since emission); a hop over a watched edge is timed now + the
        latency of the route before it, an arrival at a watched vertex now + the latency up to and
        with the hop.  Bin b covers [t0 + b * bin_ns, t0 + (b + 1) * bin_ns).  Returns a dict:
        ``hits``, the number of hits in range or not (link_crossings' total); uint64 arrays
        ``edge_fwd[ne][nbins]`` (hops leaving eu[e]; self loops; every arc of a directed
        topology), ``edge_rev[ne][nbins]`` and ``vertex[nv][nbins]``; and ``outside``, a dict of
        the same three keys with [rows][2] arrays: the weight before t0 and at or after the last
        bin."""
        s = np.ascontiguousarray(src_ips, dtype=np.uint32)
        d = np.ascontiguousarray(dst_ips, dtype=np.uint32)
        if s.shape != d.shape or s.ndim != 1:
            raise ValueError("src_ips and dst_ips must be 1-D and of one length")
        n = len(s)
        w = t = None
        if weight is not None:
            w = np.ascontiguousarray(weight, dtype=np.uint64)
            if w.shape != s.shape:
                raise ValueError("weight must have one entry per flow")
        if now is not None:
            t = np.ascontiguousarray(now, dtype=np.uint64)
            if t.shape != s.shape:
                raise ValueError("now must have one entry per flow")
        we = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1)
        wv = np.ascontiguousarray(vertices, dtype=np.int32).reshape(-1)
        ne, nv, nbins = len(we), len(wv), int(nbins)
        rows = 2 * ne + nv
        bins = np.zeros((rows, max(nbins, 0)), np.uint64)
        outside = np.zeros((rows, 2), np.uint64)
        hits = int(self._lib.shdtopo_link_timeline(
            self._h, _p(s), _p(d), _p(w) if w is not None else None,
            _p(t) if t is not None else None, n, _p(we) if ne else None, ne,
            _p(wv) if nv else None, nv, int(t0), int(bin_ns), nbins,
            _p(bins) if bins.size else None, _p(outside) if rows else None))
        if hits < 0:
            raise RuntimeError("shdtopo_link_timeline failed: %d" % hits)
        split = lambda x: {"edge_fwd": x[:ne], "edge_rev": x[ne:2 * ne], "vertex": x[2 * ne:]}
        out = split(bins)
        out["outside"] = split(outside)
        out["hits"] = hits
        return out

    def link_timeline_stats(self):
        """The last link_timeline's own counters (shdtopo_link_timeline_stats)."""
        s = L.ShdTimelineStats()
        if self._lib.shdtopo_link_timeline_stats(self._h, ctypes.byref(s)) != 0:
            raise RuntimeError("shdtopo_link_timeline_stats failed")
        return {k: getattr(s, k) for k, _ in L.ShdTimelineStats._fields_}

    # ---- link monitor ----
    def link_monitor(self, edges=(), vertices=(), t0=0, bin_ns=1_000_000, nbins=0):
        """shdtopo_monitor_new: a LinkMonitor of this topology -- link_timeline's watches and bins
        kept across calls and fed by packet windows (host arrays or the device arrays of
        route_batch_device) without walking a route."""
        return LinkMonitor(self, edges, vertices, t0, bin_ns, nbins)

    # ---- traffic matrix ----
    def traffic_matrix(self):
        """shdtopo_matrix_new: a TrafficMatrix of this topology -- packets and weight summed per
        (source vertex, destination vertex) over every fed window, exported as flows."""
        return TrafficMatrix(self)

    def vertex_ips(self, vertices):
        """shdtopo_vertex_ips: per vertex the attached IP (network order) that is lowest when
        read in host byte order, 0 for a vertex without hosts."""
        v = np.ascontiguousarray(vertices, dtype=np.int32).reshape(-1)
        ip = np.zeros(len(v), np.uint32)
        r = int(self._lib.shdtopo_vertex_ips(self._h, _p(v) if len(v) else None, len(v),
                                             _p(ip) if len(v) else None))
        if r < 0:
            raise ValueError("shdtopo_vertex_ips failed: %d" % r)
        return ip

    # ---- link failure what-if ----
    def without(self, edges=(), vertices=()):
        """shdtopo_derive_without: a new, independent Topology without the given edges (edge ids)
        and vertices (vertex ids; they lose every incident edge and stay behind isolated), with
        every attached host carried over to the same vertex.  Edge ids of the result are this
        topology's with the removed ones squeezed out (``edge_origin()`` maps them back).  Raises
        ValueError carrying the error code (``.args[1]``): -1 bad ids, -2 a failed vertex has a
        host, -3 the rest would not stay strongly connected."""
        fe = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1)
        fv = np.ascontiguousarray(vertices, dtype=np.int32).reshape(-1)
        err = ctypes.c_int32(0)
        h = self._lib.shdtopo_derive_without(self._h, _p(fe) if len(fe) else None, len(fe),
                                             _p(fv) if len(fv) else None, len(fv),
                                             ctypes.byref(err))
        if not h:
            raise ValueError("shdtopo_derive_without failed: %d" % err.value, err.value)
        return Topology(h)

    def edge_origin(self):
        """shdtopo_edge_origin: per edge id its id in the root topology (the loaded or synthesised
        one); the identity unless this topology was derived by ``without``."""
        E = int(self._lib.shdtopo_edge_origin(self._h, None, 0))
        out = np.empty(max(E, 1), np.int32)
        self._lib.shdtopo_edge_origin(self._h, _p(out), E)
        return out[:E]

    def table_diff(self, other, cap=None):
        """shdtopo_table_diff: the pairs whose {latency, reliability, hops} differ between this
        topology's table (lat0 / rel0 / hops0) and ``other``'s (lat1 / rel1 / hops1), compared on
        the device; both must have the same attached vertices.  Returns a dict: ``total``, the
        number of changed pairs; ``records`` (TABLE_CHANGE_DTYPE), the first min(total, cap) of
        them ordered by srcCol then dstCol (cap=None sizes the buffer with a cap = 0 call first);
        ``kind_count`` uint64[4], the pairs with kind bit 1, 2, 4, 8 (latency rose, latency fell,
        reliability changed, hops changed); per row ``row_changed`` uint32[A], ``row_worst_rise``
        float64[A] (the largest lat1 - lat0) and ``row_worst_col`` int32[A] (the lowest column
        reaching it; 0.0 and -1 when no latency of the row rises)."""
        kind = np.zeros(4, np.uint64)

        def call(out, c, rows):
            return int(self._lib.shdtopo_table_diff(
                self._h, other._h, _p(out) if c else None, c, _p(kind),
                _p(rows[0]) if rows else None, _p(rows[1]) if rows else None,
                _p(rows[2]) if rows else None))
        if cap is None:
            cap = call(None, 0, None)
            if cap < 0:
                raise RuntimeError("shdtopo_table_diff failed: %d" % cap, cap)
        cap = int(cap)
        A = int(self._lib.shdtopo_num_attached(self._h))
        rows = (np.zeros(max(A, 1), np.uint32), np.zeros(max(A, 1), np.float64),
                np.full(max(A, 1), -1, np.int32))
        records = np.zeros(max(cap, 1), TABLE_CHANGE_DTYPE)
        total = call(records, cap, rows)
        if total < 0:
            raise RuntimeError("shdtopo_table_diff failed: %d" % total, total)
        return {"total": total, "records": records[:min(total, cap)], "kind_count": kind,
                "row_changed": rows[0][:A], "row_worst_rise": rows[1][:A],
                "row_worst_col": rows[2][:A]}

    def table_diff_stats(self):
        """The last table_diff's own counters, kept by its first topology
        (shdtopo_table_diff_stats)."""
        s = L.ShdDiffStats()
        if self._lib.shdtopo_table_diff_stats(self._h, ctypes.byref(s)) != 0:
            raise RuntimeError("shdtopo_table_diff_stats failed")
        return {k: getattr(s, k) for k, _ in L.ShdDiffStats._fields_}

    def _flow_impact(self, what, call, n, rise_edges_ns, cap):
        """The outputs of one shdtopo_flow_impact* call; call(edges, nb, out, cap, totals,
        rise_count, rise_weight, src_w, dst_w) makes it."""
        edges = np.ascontiguousarray(rise_edges_ns, dtype=np.uint64).reshape(-1)
        nb = len(edges)
        pe = _p(edges) if nb else None
        if cap is None:
            cap = int(call(pe, nb, None, 0, None, None, None, None, None))
            if cap < 0:
                raise RuntimeError("%s failed: %d" % (what, cap), cap)
        cap = int(cap)
        A = int(self._lib.shdtopo_num_attached(self._h))
        tt = L.ShdImpactTotals()
        hist = np.zeros((2, nb + 1), np.uint64)
        colw = np.zeros((2, max(A, 1)), np.uint64)
        records = np.zeros(max(cap, 1), FLOW_CHANGE_DTYPE)
        total = int(call(pe, nb, _p(records) if cap else None, cap, ctypes.byref(tt),
                         _p(hist[0]), _p(hist[1]), _p(colw[0]), _p(colw[1])))
        if total < 0:
            raise RuntimeError("%s failed: %d" % (what, total), total)
        totals = {}
        for k, _ in L.ShdImpactTotals._fields_:
            v = getattr(tt, k)
            totals[k] = np.array(list(v), np.uint64) if k.startswith("kind") else v
        return {"total": total, "records": records[:min(total, cap)], "totals": totals,
                "rise_count": hist[0], "rise_weight": hist[1],
                "src_changed_weight": colw[0][:A], "dst_changed_weight": colw[1][:A]}

    def flow_impact(self, other, src_ips, dst_ips, weight=None, rise_edges_ns=(), cap=None):
        """shdtopo_flow_impact: what changes for the flows (src_ips[i] -> dst_ips[i], weight[i];
        None: 1 each) between this topology's table (lat0 / rel0 / hops0) and ``other``'s, joined
        on the device; both must have the same attached vertices.  Returns a dict: ``total``, the
        number of changed flows; ``records`` (FLOW_CHANGE_DTYPE), the first min(total, cap) of
        them in ascending flow order (cap=None sizes the buffer with a cap = 0 call first);
        ``totals``, the fields of ShdImpactTotals (kindCount / kindWeight as uint64[4]);
        ``rise_count`` / ``rise_weight`` uint64[len(rise_edges_ns) + 1], the histogram of the
        delay rises in ns (a rise equal to an edge goes to the upper bin);
        ``src_changed_weight`` / ``dst_changed_weight`` uint64[A], the weight of the changed flows
        leaving / entering each column.  Every sum is a u64 that wraps."""
        s = np.ascontiguousarray(src_ips, dtype=np.uint32)
        d = np.ascontiguousarray(dst_ips, dtype=np.uint32)
        if s.shape != d.shape or s.ndim != 1:
            raise ValueError("src_ips and dst_ips must be 1-D and of one length")
        w = None
        if weight is not None:
            w = np.ascontiguousarray(weight, dtype=np.uint64)
            if w.shape != s.shape:
                raise ValueError("weight must have one entry per flow")
        n = len(s)

        def call(*outs):
            return self._lib.shdtopo_flow_impact(
                self._h, other._h, _p(s) if n else None, _p(d) if n else None,
                _p(w) if w is not None else None, n, *outs)
        return self._flow_impact("shdtopo_flow_impact", call, n, rise_edges_ns, cap)

    def flow_impact_device(self, other, src_col, dst_col, payload=None, rise_edges_ns=(), cap=None,
                           stream=0):
        """shdtopo_flow_impact_device: flow_impact on the device arrays of route_batch_device
        (torch tensors used as plain HBM buffers: int32 columns, a column outside [0, A) is
        unattached; uint32-sized payload as the weight, None: 1 each).  The kernels run on
        ``stream``; the call returns when they are done."""
        n = int(src_col.numel())
        if int(dst_col.numel()) != n or (payload is not None and int(payload.numel()) != n):
            raise ValueError("the columns and the payload must be of one length")

        def call(*outs):
            return self._lib.shdtopo_flow_impact_device(
                self._h, other._h, src_col.data_ptr() if n else None,
                dst_col.data_ptr() if n else None,
                payload.data_ptr() if payload is not None else None, n, *outs, stream or None)
        return self._flow_impact("shdtopo_flow_impact_device", call, n, rise_edges_ns, cap)

    def flow_impact_stats(self):
        """The last flow_impact's own counters, kept by its first topology
        (shdtopo_flow_impact_stats); ``tile_flows`` is the build's tile, 256 x U flows."""
        s = L.ShdImpactStats()
        if self._lib.shdtopo_flow_impact_stats(self._h, ctypes.byref(s)) != 0:
            raise RuntimeError("shdtopo_flow_impact_stats failed")
        return {k: getattr(s, k) for k, _ in L.ShdImpactStats._fields_}

    def load_shift(self, other, src_ips, dst_ips, weight=None, cap=None):
        """shdtopo_load_shift: where the load of the flows (src_ips[i] -> dst_ips[i], weight[i];
        None: 1 each) differs between this topology (``before``) and ``other`` (``after``), both
        accumulated as link_load does and compared on the device in the root topology's numbering
        (``edge_origin()``).  With R root edges and V vertices, entry x < R is the forward half of
        root edge x, R <= x < 2 R the reverse half of root edge x - R, x >= 2 R vertex x - 2 R.
        Returns a dict: ``total``, the number of changed entries; ``records``
        (LOAD_CHANGE_DTYPE: kind 0 / 1 / 2, id, idA / idB = the edge's id in this topology / in
        ``other``, -1 where it lacks the edge), the first min(total, cap) in ascending x (cap=None
        sizes the buffer with a cap = 0 call first); and the fields of ShdShiftTotals (the
        per-kind ones as arrays of 3).  Every sum is a u64 that wraps."""
        s = np.ascontiguousarray(src_ips, dtype=np.uint32)
        d = np.ascontiguousarray(dst_ips, dtype=np.uint32)
        if s.shape != d.shape or s.ndim != 1:
            raise ValueError("src_ips and dst_ips must be 1-D and of one length")
        w = None
        if weight is not None:
            w = np.ascontiguousarray(weight, dtype=np.uint64)
            if w.shape != s.shape:
                raise ValueError("weight must have one entry per flow")
        n = len(s)

        def call(out, c, totals):
            return int(self._lib.shdtopo_load_shift(
                self._h, other._h, _p(s) if n else None, _p(d) if n else None,
                _p(w) if w is not None else None, n, out, c, totals))
        if cap is None:
            cap = call(None, 0, None)
            if cap < 0:
                raise RuntimeError("shdtopo_load_shift failed: %d" % cap, cap)
        cap = int(cap)
        tt = L.ShdShiftTotals()
        records = np.zeros(max(cap, 1), LOAD_CHANGE_DTYPE)
        total = call(_p(records) if cap else None, cap, ctypes.byref(tt))
        if total < 0:
            raise RuntimeError("shdtopo_load_shift failed: %d" % total, total)
        res = {"total": total, "records": records[:min(total, cap)]}
        for k, t in L.ShdShiftTotals._fields_:
            v = getattr(tt, k)
            if isinstance(v, ctypes.Array):
                v = np.array(list(v), np.uint64 if t._type_ is L.u64 else np.int64)
            res[k] = v
        return res

    def load_shift_stats(self):
        """The last load_shift's own counters, kept by its first topology
        (shdtopo_load_shift_stats); ``loadA`` / ``loadB`` are dicts with the fields of
        link_load_stats for each side's accumulation, ``tile_entries`` is the build's tile,
        256 x U entries."""
        s = L.ShdShiftStats()
        if self._lib.shdtopo_load_shift_stats(self._h, ctypes.byref(s)) != 0:
            raise RuntimeError("shdtopo_load_shift_stats failed")
        out = {k: getattr(s, k) for k, _ in L.ShdShiftStats._fields_}
        for side in ("loadA", "loadB"):
            out[side] = {k: getattr(out[side], k) for k, _ in L.ShdLoadStats._fields_}
        return out

    def write_graphml(self, path):
        if self._lib.shdtopo_write_graphml(self._h, path.encode()) != 0:
            raise RuntimeError("write_graphml failed")

    # ---- device-level boundary (torch tensors are used as plain HBM buffers) ----
    def build_rows_into(self, row0, row1, lr, hops, rowmin=None, stream=0):
        r = self._lib.shdtopo_build_rows(self._h, int(row0), int(row1), lr.data_ptr(),
                                         hops.data_ptr(),
                                         rowmin.data_ptr() if rowmin is not None else None,
                                         stream or None)
        if r != 0:
            raise RuntimeError("shdtopo_build_rows failed: %d" % r)

    def rebuild(self):
        """shdtopo_rebuild: build the whole table now (the getters build it lazily)."""
        r = self._lib.shdtopo_rebuild(self._h)
        if r != 0:
            raise RuntimeError("shdtopo_rebuild failed: %d" % r)

    def bind_table_ref(self, lr, hops, global_min, stream=0):
        """Install lr / hops in place (the tensors must outlive the binding)."""
        r = self._lib.shdtopo_bind_table_ref(self._h, lr.data_ptr(), hops.data_ptr(),
                                             float(global_min), stream or None)
        if r != 0:
            raise RuntimeError("shdtopo_bind_table_ref failed: %d" % r)
        self._bound = (lr, hops)  # keep the buffers alive while bound

    def bind_table(self, lr, hops, global_min, stream=0):
        r = self._lib.shdtopo_bind_table(self._h, lr.data_ptr(), hops.data_ptr(),
                                         float(global_min), stream or None)
        if r != 0:
            raise RuntimeError("shdtopo_bind_table failed: %d" % r)

    def route_batch_vertices(self, src_v, dst_v, payload, rng_state, now, jump_ns, clamp=True):
        """shdtopo_route_batch_vertices: (time, delivered, state, not-routed count)."""
        n = len(src_v)
        c = lambda x, t: np.ascontiguousarray(x, dtype=t)
        sv, dv = c(src_v, np.int32), c(dst_v, np.int32)
        pay, st, nw = c(payload, np.uint32), c(rng_state, np.uint32), c(now, np.uint64)
        outs = (L.TopoPacketOut * max(n, 1))()
        r = self._lib.shdtopo_route_batch_vertices(self._h, _p(sv), _p(dv), _p(pay), _p(st),
                                                   _p(nw), n, int(jump_ns), int(clamp), outs)
        if r < 0:
            raise RuntimeError("shdtopo_route_batch_vertices failed: %d" % r)
        t = np.array([outs[i].time for i in range(n)], dtype=np.uint64)
        s = np.array([outs[i].rngState for i in range(n)], dtype=np.uint32)
        dl = np.array([outs[i].delivered for i in range(n)], dtype=np.uint8)
        return t, dl, s, r

    def route_batch_device_slot(self, slot, src_col, dst_col, payload, state_in, now, jump_ns,
                                clamp, t_out, state_out, delivered, stream=0):
        r = self._lib.shdtopo_route_batch_device_slot(
            self._h, int(slot), src_col.data_ptr(), dst_col.data_ptr(), payload.data_ptr(),
            state_in.data_ptr(), now.data_ptr(), int(src_col.numel()), int(jump_ns), int(clamp),
            t_out.data_ptr(), state_out.data_ptr(), delivered.data_ptr(), stream or None)
        if r != 0:
            raise RuntimeError("shdtopo_route_batch_device_slot failed: %d" % r)

    def route_batch_device(self, src_col, dst_col, payload, state_in, now, jump_ns, clamp,
                           t_out, state_out, delivered, stream=0):
        r = self._lib.shdtopo_route_batch_device(
            self._h, src_col.data_ptr(), dst_col.data_ptr(), payload.data_ptr(),
            state_in.data_ptr(), now.data_ptr(), int(src_col.numel()), int(jump_ns), int(clamp),
            t_out.data_ptr(), state_out.data_ptr(), delivered.data_ptr(), stream or None)
        if r != 0:
            raise RuntimeError("shdtopo_route_batch_device failed: %d" % r)

    def synth_packets(self, seed, n_hosts, n_packets, t0, jump):
        """C5 workload: attach n_hosts Tor-like hosts and emit one window of packets."""
        n = int(n_packets)
        out = dict(src_col=np.empty(n, np.int32), dst_col=np.empty(n, np.int32),
                   payload=np.empty(n, np.uint32), state_in=np.empty(n, np.uint32),
                   now=np.empty(n, np.uint64), src_ip=np.empty(n, np.uint32),
                   dst_ip=np.empty(n, np.uint32))
        r = self._lib.shdtopo_synth_packets(
            self._h, int(seed), int(n_hosts), n, int(t0), int(jump), _p(out["src_col"]),
            _p(out["dst_col"]), _p(out["payload"]), _p(out["state_in"]), _p(out["now"]),
            _p(out["src_ip"]), _p(out["dst_ip"]))
        if r != 0:
            raise RuntimeError("shdtopo_synth_packets failed: %d" % r)
        return out


class LinkMonitor:
    """A link monitor (include/shd_topology_abi.h, "link monitor"): after any sequence of feeds,
    ``read()`` is what ``Topology.link_timeline`` returns for all fed packets at once."""

    def __init__(self, topology, edges=(), vertices=(), t0=0, bin_ns=1_000_000, nbins=0):
        self._top = topology
        self._lib = topology._lib
        we = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1)
        wv = np.ascontiguousarray(vertices, dtype=np.int32).reshape(-1)
        self.ne, self.nv, self.nbins = len(we), len(wv), int(nbins)
        self.id = int(self._lib.shdtopo_monitor_new(
            topology._h, _p(we) if self.ne else None, self.ne, _p(wv) if self.nv else None,
            self.nv, int(t0), int(bin_ns), self.nbins))
        if self.id < 0:
            raise RuntimeError("shdtopo_monitor_new failed: %d" % self.id)

    def _check(self, r, what):
        if r < 0:
            raise RuntimeError("shdtopo_monitor_%s failed: %d" % (what, r))
        return r

    def prepare(self):
        """Build (or rebuild) the hit index for the current columns; the number of records."""
        return self._check(int(self._lib.shdtopo_monitor_prepare(self._top._h, self.id)),
                           "prepare")

    def _feed(self, fn, what, a, b, dtype, now, weight, delivered):
        s = np.ascontiguousarray(a, dtype=dtype)
        d = np.ascontiguousarray(b, dtype=dtype)
        if s.shape != d.shape or s.ndim != 1:
            raise ValueError("the two ends must be 1-D and of one length")
        opt = []
        for x, t, name in ((weight, np.uint64, "weight"), (now, np.uint64, "now"),
                           (delivered, np.uint8, "delivered")):
            if x is not None:
                x = np.ascontiguousarray(x, dtype=t)
                if x.shape != s.shape:
                    raise ValueError("%s must have one entry per packet" % name)
            opt.append(x)
        w, t, dl = opt
        return self._check(int(fn(self._top._h, self.id, _p(s), _p(d),
                                  _p(w) if w is not None else None,
                                  _p(t) if t is not None else None,
                                  _p(dl) if dl is not None else None, len(s))), what)

    def feed(self, src_ips, dst_ips, now=None, weight=None, delivered=None):
        """Feed packets given by host IPs (numpy / sequences); this feed's hits."""
        return self._feed(self._lib.shdtopo_monitor_feed, "feed", src_ips, dst_ips, np.uint32,
                          now, weight, delivered)

    def feed_vertices(self, src_v, dst_v, now=None, weight=None, delivered=None):
        """The same by original vertex ids (-1: not attached)."""
        return self._feed(self._lib.shdtopo_monitor_feed_vertices, "feed_vertices", src_v, dst_v,
                          np.int32, now, weight, delivered)

    def feed_device(self, src_col, dst_col, now, payload=None, delivered=None, stream=0):
        """Feed the device arrays of route_batch_device (torch tensors used as plain HBM buffers:
        int32 columns, uint64-sized now, uint32-sized payload, uint8 delivered).  Enqueued on
        ``stream``, not awaited."""
        ptr = lambda x: x.data_ptr() if x is not None else None
        self._check(int(self._lib.shdtopo_monitor_feed_device(
            self._top._h, self.id, src_col.data_ptr(), dst_col.data_ptr(), ptr(payload), ptr(now),
            ptr(delivered), int(src_col.numel()), stream or None)), "feed_device")

    def read(self):
        """The cumulative bins: the dict link_timeline returns (``hits``: the cumulative hits)."""
        ne, nv, nbins = self.ne, self.nv, self.nbins
        rows = 2 * ne + nv
        bins = np.zeros((rows, max(nbins, 0)), np.uint64)
        outside = np.zeros((rows, 2), np.uint64)
        self._check(int(self._lib.shdtopo_monitor_read(
            self._top._h, self.id, _p(bins) if bins.size else None,
            _p(outside) if rows else None)), "read")
        split = lambda x: {"edge_fwd": x[:ne], "edge_rev": x[ne:2 * ne], "vertex": x[2 * ne:]}
        out = split(bins)
        out["outside"] = split(outside)
        out["hits"] = self.stats()["hits"]
        return out

    def reset(self):
        self._check(int(self._lib.shdtopo_monitor_reset(self._top._h, self.id)), "reset")

    def stats(self):
        s = L.ShdMonitorStats()
        self._check(int(self._lib.shdtopo_monitor_stats(self._top._h, self.id, ctypes.byref(s))),
                    "stats")
        return {k: getattr(s, k) for k, _ in L.ShdMonitorStats._fields_}

    def export_index(self):
        """Test hook: ``(pair_off int64[A*A + 1], row int32[R], off_ns uint64[R])`` -- pair
        (s, d) owns records [pair_off[s*A + d], pair_off[s*A + d + 1]) in hop order."""
        n = self._check(int(self._lib.shdtopo_monitor_export_index(
            self._top._h, self.id, None, None, None, 0)), "export_index")
        pairs = self.stats()["index_pairs"]
        off = np.zeros(pairs + 1, np.int64)
        row = np.zeros(max(n, 1), np.int32)
        ns = np.zeros(max(n, 1), np.uint64)
        if pairs:
            self._check(int(self._lib.shdtopo_monitor_export_index(
                self._top._h, self.id, _p(off), _p(row), _p(ns), n)), "export_index")
        return off, row[:n], ns[:n]

    def free(self):
        if self.id >= 0:
            self._lib.shdtopo_monitor_free(self._top._h, self.id)
            self.id = -1


MATRIX_FLOW = np.dtype([("srcVertex", np.int32), ("dstVertex", np.int32), ("srcIndex", np.int32),
                        ("dstIndex", np.int32), ("packets", np.uint64), ("weight", np.uint64)])


class TrafficMatrix:
    """A traffic matrix (include/shd_topology_abi.h, "traffic matrix"): after any sequence of
    feeds, ``read()`` is the per-(source vertex, destination vertex) sum of all fed packets and
    ``flows()`` the same as flows the analysis calls (link_load, flow_impact, ...) accept."""

    def __init__(self, topology):
        self._top = topology
        self._lib = topology._lib
        self.id = int(self._lib.shdtopo_matrix_new(topology._h))
        if self.id < 0:
            raise RuntimeError("shdtopo_matrix_new failed: %d" % self.id)

    def _check(self, r, what):
        if r < 0:
            raise RuntimeError("shdtopo_matrix_%s failed: %d" % (what, r), r)
        return r

    def _feed(self, fn, what, a, b, dtype, weight, delivered):
        s = np.ascontiguousarray(a, dtype=dtype)
        d = np.ascontiguousarray(b, dtype=dtype)
        if s.shape != d.shape or s.ndim != 1:
            raise ValueError("the two ends must be 1-D and of one length")
        opt = []
        for x, t, name in ((weight, np.uint64, "weight"), (delivered, np.uint8, "delivered")):
            if x is not None:
                x = np.ascontiguousarray(x, dtype=t)
                if x.shape != s.shape:
                    raise ValueError("%s must have one entry per packet" % name)
            opt.append(x)
        w, dl = opt
        return self._check(int(fn(self._top._h, self.id, _p(s), _p(d),
                                  _p(w) if w is not None else None,
                                  _p(dl) if dl is not None else None, len(s))), what)

    def feed(self, src_ips, dst_ips, weight=None, delivered=None):
        """Feed packets given by host IPs (numpy / sequences); the packets this feed counted."""
        return self._feed(self._lib.shdtopo_matrix_feed, "feed", src_ips, dst_ips, np.uint32,
                          weight, delivered)

    def feed_vertices(self, src_v, dst_v, weight=None, delivered=None):
        """The same by original vertex ids (-1: not attached)."""
        return self._feed(self._lib.shdtopo_matrix_feed_vertices, "feed_vertices", src_v, dst_v,
                          np.int32, weight, delivered)

    def feed_device(self, src_col, dst_col, payload=None, delivered=None, stream=0):
        """Feed the device arrays of route_batch_device (torch tensors used as plain HBM buffers:
        int32 columns, uint32-sized payload, uint8 delivered).  Enqueued on ``stream``, not
        awaited."""
        ptr = lambda x: x.data_ptr() if x is not None else None
        self._check(int(self._lib.shdtopo_matrix_feed_device(
            self._top._h, self.id, src_col.data_ptr(), dst_col.data_ptr(), ptr(payload),
            ptr(delivered), int(src_col.numel()), stream or None)), "feed_device")

    def vertices(self):
        """The matrix's vertex list mv (ascending original vertex ids)."""
        m = self._check(int(self._lib.shdtopo_matrix_vertices(self._top._h, self.id, None, 0)),
                        "vertices")
        out = np.zeros(m, np.int32)
        if m:
            self._check(int(self._lib.shdtopo_matrix_vertices(self._top._h, self.id, _p(out), m)),
                        "vertices")
        return out

    def read(self, cap=None):
        """``(records, sums, totals)``: the reported cells (a MATRIX_FLOW structured array in
        ascending (srcVertex, dstVertex) order, the first ``cap`` of them when given), a dict of
        the four u64[M] sum arrays (sentPackets, sentWeight, recvPackets, recvWeight) and a dict
        of ShdMatrixTotals (``cells`` counts every reported cell whatever ``cap`` is)."""
        h, lib = self._top._h, self._lib
        if cap is None:
            cap = self._check(int(lib.shdtopo_matrix_read(h, self.id, None, 0, None, None, None,
                                                          None, None)), "read")
        cap = int(cap)
        m = len(self.vertices())
        rec = np.zeros(max(cap, 1), MATRIX_FLOW)
        names = ("sentPackets", "sentWeight", "recvPackets", "recvWeight")
        sums = {k: np.zeros(m, np.uint64) for k in names}
        tot = L.ShdMatrixTotals()
        n = self._check(int(lib.shdtopo_matrix_read(
            h, self.id, _p(rec) if cap else None, cap,
            *[_p(sums[k]) if m else None for k in names], ctypes.byref(tot))), "read")
        return (rec[:min(n, cap)], sums,
                {k: getattr(tot, k) for k, _ in L.ShdMatrixTotals._fields_})

    def flows(self, cap=None):
        """``(src_ips, dst_ips, weight, packets)`` of the reported cells, each vertex standing
        in with its lowest attached IP (Topology.vertex_ips): what link_load, link_crossings,
        link_timeline, flow_impact and load_shift accept.  Records whose source or destination
        vertex has no host any more are dropped; ``self.dropped`` is their number."""
        rec, _, _ = self.read(cap)
        ips = self._top.vertex_ips(self.vertices())
        s, d = ips[rec["srcIndex"]], ips[rec["dstIndex"]]
        keep = (s != 0) & (d != 0)
        self.dropped = int(len(rec) - keep.sum())
        return (s[keep], d[keep], np.ascontiguousarray(rec["weight"][keep]),
                np.ascontiguousarray(rec["packets"][keep]))

    def reset(self):
        self._check(int(self._lib.shdtopo_matrix_reset(self._top._h, self.id)), "reset")

    def stats(self):
        s = L.ShdMatrixStats()
        self._check(int(self._lib.shdtopo_matrix_stats(self._top._h, self.id, ctypes.byref(s))),
                    "stats")
        return {k: getattr(s, k) for k, _ in L.ShdMatrixStats._fields_}

    def free(self):
        if self.id >= 0:
            self._lib.shdtopo_matrix_free(self._top._h, self.id)
            self.id = -1


PACKET_IN = np.dtype([("srcIP", np.uint32), ("dstIP", np.uint32), ("payloadLength", np.uint32),
                      ("rngState", np.uint32), ("now", np.uint64)])
PACKET_OUT = np.dtype([("time", np.uint64), ("rngState", np.uint32), ("delivered", np.uint8),
                       ("_pad", np.uint8, 3)])


class RouteSchedule:
    """A route schedule (include/shd_topology_abi.h, "route schedule"): ``tops[e]`` routes the
    packets emitted at or after ``from_ns[e]`` and before ``from_ns[e + 1]``; ``from_ns[0]`` is 0
    and the start times ascend strictly.  The same topology may appear in several epochs, as in
    ``[parent, child, parent]`` for a link that fails and comes back; every member needs the
    attached vertices of ``tops[0]``.  The library validates the schedule at every call."""

    def __init__(self, tops, from_ns):
        self.tops = list(tops)
        self.from_ns = np.ascontiguousarray(from_ns, dtype=np.uint64).reshape(-1)
        if len(self.tops) != len(self.from_ns):
            raise ValueError("one start time per topology")
        self.k = len(self.tops)
        self._lib = L.load()[0]
        self._handles = (ctypes.c_void_p * max(self.k, 1))(
            *[t._h if t is not None else None for t in self.tops])

    def _check(self, r, what):
        if r < 0:
            raise RuntimeError("%s failed: %d" % (what, r), r)
        return int(r)

    def _host(self, what, call, n, want_epoch):
        out = np.zeros(max(n, 1), PACKET_OUT)
        epoch = np.zeros(max(n, 1), np.uint8) if want_epoch else None
        count = np.zeros((max(self.k, 1), 3), np.uint64)
        r = self._check(call(_p(out), _p(epoch) if want_epoch else None, _p(count)), what)
        out = out[:n]
        return (out["time"].copy(), out["delivered"].copy(), out["rngState"].copy(),
                epoch[:n] if want_epoch else None, count[:self.k], r)

    def route(self, src_ip, dst_ip, payload, rng_state, now, jump_ns, clamp=True, epoch=True):
        """shdtopo_route_schedule: (time, delivered, state, epoch, epoch_count, not_routed) of the
        packets given by their hosts' IPs, resolved through ``tops[0]``."""
        n = len(src_ip)
        ins = np.zeros(max(n, 1), PACKET_IN)
        for name, x in (("srcIP", src_ip), ("dstIP", dst_ip), ("payloadLength", payload),
                        ("rngState", rng_state), ("now", now)):
            ins[name][:n] = x
        return self._host("shdtopo_route_schedule", lambda out, ep, cnt:
                          self._lib.shdtopo_route_schedule(
                              self._handles, _p(self.from_ns), self.k, _p(ins), out, n,
                              int(jump_ns), int(clamp), ep, cnt), n, epoch)

    def route_vertices(self, src_v, dst_v, payload, rng_state, now, jump_ns, clamp=True,
                       epoch=True):
        """shdtopo_route_schedule_vertices: the same for packets given by their vertices."""
        n = len(src_v)
        c = lambda x, t: np.ascontiguousarray(x, dtype=t)
        sv, dv = c(src_v, np.int32), c(dst_v, np.int32)
        pay, st, nw = c(payload, np.uint32), c(rng_state, np.uint32), c(now, np.uint64)
        return self._host("shdtopo_route_schedule_vertices", lambda out, ep, cnt:
                          self._lib.shdtopo_route_schedule_vertices(
                              self._handles, _p(self.from_ns), self.k, _p(sv), _p(dv), _p(pay),
                              _p(st), _p(nw), n, int(jump_ns), int(clamp), out, ep, cnt), n, epoch)

    def route_device(self, src_col, dst_col, payload, state_in, now, jump_ns, clamp, t_out,
                     state_out, delivered, epoch=None, stream=0):
        """shdtopo_route_schedule_device on the device arrays of Topology.route_batch_device
        (torch tensors used as plain HBM buffers); ``epoch``: an optional uint8 tensor that
        receives each packet's epoch.  The kernel runs on ``stream``; the call returns when it is
        done.  Returns epoch_count, uint64 [k, 3]: packets, delivered, not routed per epoch."""
        n = int(src_col.numel())
        count = np.zeros((max(self.k, 1), 3), np.uint64)
        ptr = lambda x: x.data_ptr() if n else None
        self._check(self._lib.shdtopo_route_schedule_device(
            self._handles, _p(self.from_ns), self.k, ptr(src_col), ptr(dst_col), ptr(payload),
            ptr(state_in), ptr(now), n, int(jump_ns), int(clamp), ptr(t_out), ptr(state_out),
            ptr(delivered), epoch.data_ptr() if epoch is not None and n else None, _p(count),
            stream or None), "shdtopo_route_schedule_device")
        return count[:self.k]

    def stats(self):
        """The last call's own counters, kept by ``tops[0]`` (shdtopo_route_schedule_stats)."""
        s = L.ShdScheduleStats()
        self._check(self._lib.shdtopo_route_schedule_stats(self.tops[0]._h, ctypes.byref(s)),
                    "shdtopo_route_schedule_stats")
        out = {k: getattr(s, k) for k, _ in L.ShdScheduleStats._fields_}
        for f in ("epoch_packets", "epoch_delivered"):
            out[f] = np.array(list(out[f]), np.int64)
        return out


def shim():
    return L.load()[1]
