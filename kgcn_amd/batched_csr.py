"""Batched-CSR adjacency container: the HBM layout the HIP kernels read (include/kgcn_hip.h).

The reference feeds adjacency as B x C separate tf.SparseTensorValue (indices [nnz,2], values
[nnz], dense_shape [2]) per step (kgcn/feed.py:112-126, placeholders from
kgcn/default_model.py:10).  Here one adjacency channel of the whole batch is ONE pair of device
arrays, built once per batch (or once per dataset and cached):

    rowptr int32 [T*M + 1]    absolute entry offsets, row r of graph t at index t*M + r
    cv     int32 [nnz, 2]     (column local to the graph, fp32 value bits), CSR order

Entries of a row keep their COO order (stable sort), duplicates stay separate entries (they
accumulate like in TF), dummy graphs (nnz = 0) are legal.  The transposed container (A^T of every
graph) serves adjoint_a=True, i.e. every backward pass (kgcn/bspmm_call.py:45).
"""
import ctypes

import numpy as np

from . import _lib


def _as_triple(m):
    """Accept the reference's layouts: (idx, val, shape) tuples/lists or objects exposing
    .indices/.values/.dense_shape (kgcn/bspmm_call.py:12-14)."""
    if hasattr(m, "indices") and hasattr(m, "dense_shape"):
        return m.indices, m.values, m.dense_shape
    return m[0], m[1], m[2]


def _to_numpy(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def flatten_coo_list(mats, need_shape=True):
    """T sparse matrices in the reference's per-graph COO layout -> (idx [nnz, 2] int, val [nnz] f32, counts [T] int64,
    M, K) with TWO concatenations instead of a Python loop over the matrices: kgcn/feed.py:112-126 hands over B x C separate
    SparseTensorValues built from the dataset's arrays, and walking them one by one (asarray, reshape, full, append per
    matrix) cost 10.8 ms for 4,096 graphs.  The fast path takes plain (idx ndarray [n, 2], val ndarray [n], shape)
    triples (what the reference's loaders hold, kgcn/data_util.py:40-45); anything else -- objects with .indices, torch
    tensors, ragged index shapes -- goes through the general per-matrix route.  M / K (max over the dense_shapes) are only
    scanned when `need_shape`."""
    T = len(mats)
    M = K = 0
    fast = T > 0 and all(type(m) in (tuple, list) and type(m[0]) is np.ndarray and type(m[1]) is np.ndarray
                         for m in (mats[0], mats[-1]))
    if fast:
        try:
            idxs = [m[0] for m in mats]
            vals = [m[1] for m in mats]
            counts = np.fromiter(map(len, vals), np.int64, T)
            idx = np.concatenate(idxs)
            val = np.concatenate(vals)
            if idx.ndim != 2 or idx.shape[1] != 2 or val.ndim != 1 or idx.shape[0] != val.shape[0] or \
                    int(counts.sum()) != val.shape[0] or \
                    not np.array_equal(np.fromiter(map(len, idxs), np.int64, T), counts):
                raise ValueError
            if need_shape:
                for m in mats:
                    if m[2] is not None:
                        M = max(M, int(m[2][0]))
                        K = max(K, int(m[2][1]))
            return idx, val.astype(np.float32, copy=False), counts, M, K
        except (ValueError, TypeError, IndexError):
            pass                                       # irregular input: the general route reports what is wrong
    idxs, vals, counts = [], [], np.zeros(T, np.int64)
    for t, m in enumerate(mats):
        i, v, shape = _as_triple(m)
        i = _to_numpy(i).reshape(-1, 2)
        v = _to_numpy(v).reshape(-1)
        if shape is not None:
            M = max(M, int(shape[0]))
            K = max(K, int(shape[1]))
        if i.shape[0] != v.shape[0]:
            raise ValueError("matrix %d: %d indices but %d values" % (t, i.shape[0], v.shape[0]))
        counts[t] = i.shape[0]
        idxs.append(i)
        vals.append(v)
    idx = np.concatenate(idxs) if idxs else np.zeros((0, 2), np.int64)
    val = (np.concatenate(vals) if vals else np.zeros(0, np.float32)).astype(np.float32, copy=False)
    return idx, val, counts, M, K


# from_coo_list() packs batches with at least this many stored entries on the GPU (kgcn_coo_pack_f32); smaller ones on the
# host (a handful of tiny launches and one 8-byte read-back cost more than numpy there)
DEVICE_PACK_MIN_NNZ = 20000


class BatchedCSR:
    """One adjacency channel of a batch of T graphs, device resident."""

    PAD_COL, ROW_PAD_COMPACT, UNIT_VALUES = (_lib.K[n] for n in ("KGCN_PAD_COL", "KGCN_ROW_PAD_COMPACT", "KGCN_CSR_UNIT_VALUES"))

    def __init__(self, rowptr, cv, num_graphs, rows, cols, max_nnz, perm=None, host=None,
                 row_pad=0):
        self.rowptr = rowptr            # torch int32 [T*M+1] (device)
        self.cv = cv                    # torch int32 [nnz,2] (device)
        self.num_graphs = int(num_graphs)
        self.rows = int(rows)
        self.cols = int(cols)
        self.max_nnz = int(max_nnz)
        self.nnz = int(cv.shape[0])
        self.perm = perm                # torch int64 [nnz]: CSR position -> input (COO) position
        self._host = host               # (g, r, c, v) numpy arrays in CSR order, for transpose()
        self._t = None
        self._desc = None
        self._struct_src = None         # set by with_values(): container owning the pattern
        self._vals = None
        self.row_pad = int(row_pad)     # 0 plain CSR, 4 = rows padded to multiples of 4 entries
        self._p4 = None
        self._c4 = None                 # row_pad == 4: cache of compact4() (False: the batch does not fit the compact slot)
        self._make_t = None             # thunks set by gather(): build A^T / the padded copy on demand
        self._make_p4 = None
        self._graph_counts = None       # host int64 [T]: stored entries per graph
        self._tperm = None              # cache of transpose_perm()
        self._refillable = False        # static_like(): contents change under the same object
        self.slots = None               # row_pad == 4: int32 [T*M] slot table (see include/kgcn_hip.h)
        self.graph_ptr = None           # row_pad == 4: int32 [T+1]
        self.block_ptr = None           # ragged-compact containers: int32 [num_blocks + 1] row blocks of whole molecules
        self.block_rows_max = 0         # ... and the most rows a block can hold (kgcn_csr_batch.block_ptr, include/kgcn_hip.h)

    # ---- construction -------------------------------------------------------------------------
    @classmethod
    def from_arrays(cls, graph, row, col, val, num_graphs, rows, cols, device="cuda"):
        """Build from flat COO arrays (graph id, local row, local col, value) of all graphs."""
        import torch
        graph = np.asarray(graph, np.int64).ravel()
        row = np.asarray(row, np.int64).ravel()
        col = np.asarray(col, np.int64).ravel()
        val = np.asarray(val, np.float32).ravel()
        nnz = graph.shape[0]
        if not (row.shape[0] == col.shape[0] == val.shape[0] == nnz):
            raise ValueError("graph/row/col/val length mismatch")
        T, M, K = int(num_graphs), int(rows), int(cols)
        if nnz:
            if graph.min() < 0 or graph.max() >= T:
                raise ValueError("graph id out of range")
            if row.min() < 0 or row.max() >= M:
                raise ValueError("row index out of range for %d rows" % M)
            if col.min() < 0 or col.max() >= K:
                raise ValueError("column index out of range for %d columns" % K)
        if T * M + 1 >= 2 ** 31 or nnz >= 2 ** 31:
            raise ValueError("batch too large for int32 offsets")
        key = graph * M + row
        if nnz and np.any(key[1:] < key[:-1]):
            order = np.argsort(key, kind="stable")
            graph, row, col, val, key = graph[order], row[order], col[order], val[order], key[order]
        else:
            order = None
        counts = np.bincount(key, minlength=T * M) if nnz else np.zeros(T * M, np.int64)
        rowptr = np.zeros(T * M + 1, np.int64)
        np.cumsum(counts, out=rowptr[1:])
        if T and M:
            per_graph = rowptr[M::M] - rowptr[:-1:M] if M else np.zeros(T, np.int64)
            max_nnz = int(per_graph.max()) if per_graph.size else 0
        else:
            max_nnz = 0
        cv = np.empty((nnz, 2), np.int32)
        cv[:, 0] = col
        cv[:, 1] = val.view(np.int32)
        dev = torch.device(device)
        t_rowptr = torch.from_numpy(rowptr.astype(np.int32)).to(dev)
        t_cv = torch.from_numpy(cv).to(dev)
        perm = None if order is None else torch.from_numpy(order).to(dev)
        return cls(t_rowptr, t_cv, T, M, K, max_nnz, perm=perm, host=(graph, row, col, val))

    @classmethod
    def from_device_coo(cls, graph, row, col, val, num_graphs, rows, cols, _transposed=False):
        """Build from flat COO tensors that already live on the GPU (int32 graph / row / col, fp32 val or None = ones),
        in any order, WITHOUT a host round trip of the triples: kgcn_coo_pack_f32 (stable device radix sort, rocPRIM).
        Same container, bit for bit, as from_arrays() on the same triples; transpose() and padded4() are built on the
        device too (kgcn_coo_pack_f32(transposed), kgcn_csr_pad4).  One 8-byte read-back (max entries per graph -- it
        sizes the kernels' LDS staging -- and the out-of-range count)."""
        import torch
        lib = _lib.lib
        T, M, K = int(num_graphs), int(rows), int(cols)
        dev = graph.device
        _lib.require_gpu(graph, "graph")
        g, r, c = (t.to(torch.int32).contiguous().reshape(-1) for t in (graph, row, col))
        v = None if val is None else val.to(torch.float32).contiguous().reshape(-1)
        nnz = g.numel()
        if not (r.numel() == c.numel() == nnz and (v is None or v.numel() == nnz)):
            raise ValueError("graph/row/col/val length mismatch")
        R = K if _transposed else M
        rowptr = torch.empty(T * R + 1, device=dev, dtype=torch.int32)
        cv = torch.empty((nnz, 2), device=dev, dtype=torch.int32)
        perm = torch.empty(nnz, device=dev, dtype=torch.int32)
        stats = torch.empty(2, device=dev, dtype=torch.int32)
        wsb = lib.kgcn_coo_pack_workspace_bytes(nnz, T, M, K)
        ws = _lib.workspace(wsb, dev, torch.int64)
        _lib.check(lib.kgcn_coo_pack_f32(_lib.ptr(g), _lib.ptr(r), _lib.ptr(c), _lib.ptr(v), nnz, T, M, K,
                                         1 if _transposed else 0, _lib.ptr(rowptr), cv.data_ptr() if nnz else 0,
                                         _lib.ptr(perm) if nnz else None, _lib.ptr(stats), _lib.ptr(ws), wsb,
                                         _lib.current_stream()), "kgcn_coo_pack_f32")
        max_nnz, bad = (int(x) for x in stats.tolist())
        if bad:
            raise ValueError("%d COO entries outside [0, %d) x [0, %d) x [0, %d)" % (bad, T, M, K))
        out = cls(rowptr, cv, T, R, M if _transposed else K, max_nnz, perm=perm.long())
        if not _transposed:
            def make_t():
                t = cls.from_device_coo(g, r, c, v, T, M, K, _transposed=True)
                return t
            out._make_t = make_t
        out._make_p4 = out._pad4_on_device
        return out

    def _pad4_on_device(self):
        """Row-padded copy (padded4()) of a device-built container through kgcn_csr_pad4."""
        import torch
        lib = _lib.lib
        if self.rows > self.PAD_COL or self.cols > self.PAD_COL:
            raise ValueError("row padding is only defined for graphs of at most %d nodes" % self.PAD_COL)
        T, M, dev = self.num_graphs, self.rows, self.rowptr.device
        cap = self.nnz + 4 * T * M
        rp4 = torch.empty(T * M + 1, device=dev, dtype=torch.int32)
        cv4 = torch.empty((cap, 2), device=dev, dtype=torch.int32)
        slots = torch.empty(T * M, device=dev, dtype=torch.int32)
        gptr = torch.empty(T + 1, device=dev, dtype=torch.int32)
        stats = torch.empty(3, device=dev, dtype=torch.int32)
        wsb = lib.kgcn_csr_pad4_workspace_bytes(T, M)
        ws = _lib.workspace(wsb, dev, torch.int64)
        _lib.check(lib.kgcn_csr_pad4(self.desc(), _lib.ptr(rp4), cv4.data_ptr(), cap, _lib.ptr(slots), _lib.ptr(gptr),
                                     _lib.ptr(stats), _lib.ptr(ws), wsb, _lib.current_stream()), "kgcn_csr_pad4")
        max_nnz, total, bad = (int(x) for x in stats.tolist())
        if bad or max_nnz >= 65536:
            raise ValueError("graph too dense for the packed slot table of the fused kernels")
        p4 = BatchedCSR(rp4, cv4[:total], T, M, self.cols, max_nnz, row_pad=4)
        p4.slots, p4.graph_ptr = slots, gptr
        return p4

    @classmethod
    def from_coo_list(cls, mats, rows=None, cols=None, device="cuda", _flat=None):
        """mats: T sparse matrices in the reference's COO layout (see _as_triple).  Graphs are
        padded to the common (max) shape like kgcn/data_util.py:30-37 does with max_node_num."""
        import torch
        idx, val, counts, M, K = flatten_coo_list(mats, need_shape=rows is None or cols is None) if _flat is None else _flat
        M, K = (rows if rows is not None else M), (cols if cols is not None else K)
        T = len(mats)
        nnz = int(val.shape[0])
        if nnz >= DEVICE_PACK_MIN_NNZ and torch.device(device).type == "cuda":
            # big batches: the triples are uploaded as they are ([nnz, 2] indices, values, per-graph counts) and packed on
            # the GPU (A now; A^T and the row-padded copies on demand) -- the numpy route sorts on the host for every new
            # batch (A^T always, A when the feed is unsorted)
            di = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(device)
            dv = torch.from_numpy(np.ascontiguousarray(val, dtype=np.float32)).to(device)
            dg = torch.repeat_interleave(torch.arange(T, device=device, dtype=torch.int32),
                                         torch.from_numpy(counts).to(device), output_size=nnz)
            return cls.from_device_coo(dg, di[:, 0], di[:, 1], dv, T, M, K)
        g = np.repeat(np.arange(T, dtype=np.int64), counts)
        return cls.from_arrays(g, idx[:, 0].astype(np.int64), idx[:, 1].astype(np.int64), val, T, M, K, device=device)

    # ---- derived -------------------------------------------------------------------------------
    def transpose(self):
        """Batched CSR of A[t]^T (cached).  Entry order inside a transposed row follows the
        original row-major order, i.e. ascending original row."""
        if self._t is None and self._make_t is not None:
            self._t = self._make_t()
            self._t._t = self
        if self._t is None:
            if self._struct_src is not None:
                src = self._struct_src
                bt = src.transpose()                       # pattern of A^T (cached there)
                # the values must follow the entries into A^T order.  A host-built A^T knows that order (bt.perm,
                # None = unchanged); a gathered / static container does not (its A^T is a segmented copy of the
                # dataset's A^T): there the permutation is computed on the device from the pattern itself
                if src._host is not None:
                    vt = self._vals if bt.perm is None else self._vals[bt.perm]
                else:
                    vt = self._vals[src.transpose_perm()]
                t = bt.with_values(vt)
            else:
                g, r, c, v = self._host
                t = BatchedCSR.from_arrays(g, c, r, v, self.num_graphs, self.cols, self.rows,
                                           device=self.rowptr.device)
            t._t = self
            self._t = t
        return self._t

    def transpose_perm(self):
        """Device int64 [nnz]: position in the CSR of A^T -> position in this CSR, for the entry order transpose()
        produces (entries of a transposed row in ascending original row, ties in original order).  Computed from the
        device arrays (a stable sort of the keys (graph, col, row)); cached unless the container is a refillable one."""
        import torch
        if self._tperm is not None and not self._refillable:
            return self._tperm
        if self.row_pad:
            raise NotImplementedError("transpose_perm() is defined on the plain layout")
        nnz, M, K = self.nnz, self.rows, self.cols
        dev = self.rowptr.device
        e = torch.arange(nnz, device=dev, dtype=torch.int64)
        grow = torch.searchsorted(self.rowptr[1:].long(), e, right=True)          # global row t*M + r of every entry
        key = (torch.div(grow, M, rounding_mode="floor") * K + self.cv[:, 0].long()) * M + grow % M
        perm = torch.argsort(key, stable=True)
        if not self._refillable:
            self._tperm = perm
        return perm

    def padded4(self):
        """Row-padded copy for the fused GraphConv kernels (kgcn_csr_batch.row_pad = 4): every row
        holds a positive multiple of 4 entries; padding entries are (col = PAD_COL, value = 0) and
        gather an all-zero LDS row, so the kernels run mask-free 4-entry gathers.  Cached."""
        if self.row_pad == 4:
            return self
        if self._p4 is None and self._make_p4 is not None:
            self._p4 = self._make_p4()
        if self._p4 is None:
            import torch
            if self._host is None:
                raise NotImplementedError("padded4() needs the host-side pattern (not available on "
                                          "containers made by with_values())")
            if self.rows > self.PAD_COL or self.cols > self.PAD_COL:
                raise ValueError("row padding is only defined for graphs of at most %d nodes" % self.PAD_COL)
            g, r, c, v = self._host
            T, M = self.num_graphs, self.rows
            nnz = g.shape[0]
            key = g * M + r
            counts = np.bincount(key, minlength=T * M) if nnz else np.zeros(T * M, np.int64)
            padded = np.maximum(4, (counts + 3) // 4 * 4)
            rp = np.zeros(T * M + 1, np.int64)
            np.cumsum(counts, out=rp[1:])
            rp4 = np.zeros(T * M + 1, np.int64)
            np.cumsum(padded, out=rp4[1:])
            n4 = int(rp4[-1])
            if n4 >= 2 ** 31:
                raise ValueError("batch too large for int32 offsets")
            cv4 = np.empty((n4, 2), np.int32)
            cv4[:, 0] = self.PAD_COL
            cv4[:, 1] = 0
            if nnz:
                pos = rp4[key] + (np.arange(nnz) - rp[key])
                cv4[pos, 0] = c
                cv4[pos, 1] = v.view(np.int32)
            per_graph = rp4[M::M] - rp4[:-1:M] if (T and M) else np.zeros(0, np.int64)
            max_nnz = int(per_graph.max()) if per_graph.size else 0
            if max_nnz >= 65536 or (padded.size and padded.max() > 252):
                raise ValueError("graph too dense for the packed slot table of the fused kernels")
            # slot table: per graph, rows by decreasing (padded) length, stable
            gptr = rp4[::M] if M else np.zeros(T + 1, np.int64)
            if T and M:
                plen = padded.reshape(T, M)
                order = np.argsort(-plen, axis=1, kind="stable")                 # [T, M] row ids
                start = (rp4[:-1].reshape(T, M) - gptr[:-1, None])               # local offsets
                so = np.take_along_axis(start, order, 1)
                lo = np.take_along_axis(plen, order, 1)
                slots = (so | (lo << 16) | (order << 24)).astype(np.uint32).view(np.int32).reshape(-1)
            else:
                slots = np.zeros(0, np.int32)
            dev = self.rowptr.device
            self._p4 = BatchedCSR(torch.from_numpy(rp4.astype(np.int32)).to(dev),
                                  torch.from_numpy(cv4).to(dev), T, M, self.cols, max_nnz,
                                  row_pad=4)
            self._p4.slots = torch.from_numpy(np.ascontiguousarray(slots)).to(dev)
            self._p4.graph_ptr = torch.from_numpy(gptr.astype(np.int32)).to(dev)
            self._p4._graph_counts = np.diff(gptr).astype(np.int64)
        return self._p4

    def compact4(self, build=True):
        """Compact copy of padded4() for the FULL-shape fused kernels (kgcn_csr_batch.row_pad = KGCN_ROW_PAD_COMPACT,
        include/kgcn_hip.h): the same rows, entries and padding, with one byte per column, a value stream only when
        some stored value is not 1.0f and 16-bit row slots.  Built on the device (kgcn_csr_compact4) once per batch
        and cached on the row-padded container; the build reads two counters back to the host.  Returns a
        CompactCSR, or None: the batch does not fit the 16-bit slot, the container is refilled in place
        (static_like(): a copy would go stale), or build=False and nothing is cached yet."""
        p4 = self.padded4()
        if p4._refillable or self._refillable:
            return None
        if p4._c4 is None:
            if not build:
                return None
            p4._c4 = CompactCSR.build(p4) or False
        return p4._c4 or None

    def graph_counts(self):
        """Host int64 [T]: stored entries per graph (padding entries included for row_pad = 4)."""
        if self._graph_counts is None:
            if self._host is not None:
                self._graph_counts = np.bincount(self._host[0], minlength=self.num_graphs).astype(np.int64)
            else:
                rp = self.rowptr[::self.rows].cpu().numpy().astype(np.int64) if self.rows else \
                    np.zeros(self.num_graphs + 1, np.int64)
                self._graph_counts = np.diff(rp)
        return self._graph_counts

    def gather(self, sel, out=None, sel_dev=None):
        """Mini-batch assembly ON THE DEVICE (kgcn_csr_gather_graphs): `self` is the container of the
        whole dataset, sel[t] the dataset index of batch graph t (-1 = empty dummy graph padding a short
        batch, kgcn/feed.py:123-126).  The host only adds up the selected graphs' entry counts (to size
        the output); rowptr / cv / slots never leave HBM.  A^T and the row-padded copy of the batch are
        gathered lazily from the dataset's own A^T / padded containers.

        out: a container made by static_like() -- the batch is written into its (fixed) buffers, so that a
        captured hipGraph whose kernels hold those pointers can be replayed on the new batch."""
        import torch
        if self.rowptr.device.type != "cuda":
            raise _lib.KgcnHipError("gather(): device-side batch assembly needs a device-resident container")
        if out is not None and sel_dev is not None:
            # refill of a static container (sized for the worst case, indices validated by the caller once per
            # batch): no host arithmetic at all, one kernel sequence
            T = int(sel_dev.shape[0])
            if (out.num_graphs, out.rows, out.cols, out.row_pad) != (T, self.rows, self.cols, self.row_pad):
                raise ValueError("static container does not match the batch shape")
            worst = max(self.max_nnz, 4 * self.rows if self.row_pad else 0)
            if out.nnz < T * worst or not hasattr(out, "_gptr_buf"):
                raise ValueError("refill target must come from static_like(this container, %d): it holds %d entries, "
                                 "the worst case is %d" % (T, out.nnz, T * worst))
            if sel_dev.dtype != torch.int32 or not sel_dev.is_cuda:
                raise ValueError("sel_dev must be a device int32 tensor (indices validated by the caller)")
            wsb = _lib.lib.kgcn_csr_gather_workspace_bytes(T)
            _lib.check(_lib.lib.kgcn_csr_gather_graphs(
                self.desc(), sel_dev.data_ptr(), T, out.rowptr.data_ptr(), out.cv.data_ptr() if out.nnz else 0, out.nnz,
                out.slots.data_ptr() if out.slots is not None else 0, out._gptr_buf.data_ptr(), out._ws.data_ptr(), wsb,
                _lib.current_stream()), "kgcn_csr_gather_graphs")
            out._graph_counts = None
            return out
        sel = np.asarray(sel, np.int64).reshape(-1)
        T, M = sel.shape[0], self.rows
        if T and (sel.max() >= self.num_graphs or sel.min() < -1):
            raise ValueError("graph index out of range for a dataset of %d graphs" % self.num_graphs)
        counts = self.graph_counts()
        dummy = 4 * M if self.row_pad else 0
        per = np.where(sel >= 0, counts[np.maximum(sel, 0)], dummy) if T else np.zeros(0, np.int64)
        total = int(per.sum())
        if T * M + 1 >= 2 ** 31 or total >= 2 ** 31:
            raise ValueError("batch too large for int32 offsets")
        dev = self.rowptr.device
        i32 = dict(device=dev, dtype=torch.int32)
        sel_d = torch.from_numpy(sel.astype(np.int32)).to(dev) if sel_dev is None else sel_dev
        wsb = _lib.lib.kgcn_csr_gather_workspace_bytes(T)
        if out is None:
            rowptr = torch.empty(T * M + 1, **i32)
            cv = torch.empty((total, 2), **i32)
            gptr = torch.empty(T + 1, **i32)
            slots = torch.empty(T * M, **i32) if self.row_pad else None
            ws = _lib.workspace(wsb, dev, torch.int32)
            cap = total
        else:
            if (out.num_graphs, out.rows, out.cols, out.row_pad) != (T, M, self.cols, self.row_pad):
                raise ValueError("static container does not match the batch shape")
            if total > out.nnz:
                raise ValueError("batch holds %d entries, static container only %d" % (total, out.nnz))
            rowptr, cv, gptr, slots, ws, cap = out.rowptr, out.cv, out._gptr_buf, out.slots, out._ws, out.nnz
        _lib.check(_lib.lib.kgcn_csr_gather_graphs(
            self.desc(), sel_d.data_ptr(), T, rowptr.data_ptr(), cv.data_ptr() if cap else 0, cap,
            slots.data_ptr() if slots is not None else 0, gptr.data_ptr(), ws.data_ptr(), wsb,
            _lib.current_stream()), "kgcn_csr_gather_graphs")
        if out is not None:
            out._graph_counts = per.astype(np.int64)
            return out
        res = BatchedCSR(rowptr, cv, T, M, self.cols, int(per.max()) if T else 0, row_pad=self.row_pad)
        res._graph_counts = per.astype(np.int64)
        if self.row_pad:
            res.slots, res.graph_ptr = slots, gptr
        else:
            src = self
            res._make_t = lambda: src.transpose().gather(sel)
            res._make_p4 = lambda: src.padded4().gather(sel)
        return res

    @classmethod
    def static_like(cls, src, num_graphs):
        """Fixed-address container for batches of `num_graphs` graphs gathered out of `src`: sized for the
        worst case (every graph as large as the dataset's largest), max_nnz = that bound (it only sizes the
        kernels' LDS staging), nnz = capacity.  Filled by src.gather(sel, out=...)."""
        import torch
        T, M = int(num_graphs), src.rows
        worst = max(src.max_nnz, 4 * M if src.row_pad else 0)
        dev = src.rowptr.device
        i32 = dict(device=dev, dtype=torch.int32)
        out = cls(torch.zeros(T * M + 1, **i32), torch.zeros((T * worst, 2), **i32), T, M, src.cols, worst,
                  row_pad=src.row_pad)
        out._refillable = True
        out._gptr_buf = torch.zeros(T + 1, **i32)
        out._ws = _lib.workspace(_lib.lib.kgcn_csr_gather_workspace_bytes(T), dev, torch.int32)
        if src.row_pad:
            out.slots = torch.zeros(T * M, **i32)
            out.graph_ptr = out._gptr_buf
        return out

    def with_values(self, values):
        """Same pattern, new values (device fp32 tensor [nnz] in CSR order).  Used when the
        adjacency values are themselves differentiable inputs (kgcn/bspmm_call.py:50-55)."""
        import torch
        cv = torch.stack((self.cv[:, 0], values.detach().contiguous().view(torch.int32)), dim=1)
        out = BatchedCSR(self.rowptr, cv.contiguous(), self.num_graphs, self.rows, self.cols,
                         self.max_nnz, perm=self.perm, host=None)
        out.block_ptr, out.block_rows_max = self.block_ptr, self.block_rows_max
        out._struct_src = self if self._struct_src is None else self._struct_src
        out._vals = values.detach()
        return out

    @property
    def values(self):
        import torch
        return self.cv[:, 1].contiguous().view(torch.float32)

    @property
    def device(self):
        return self.rowptr.device

    def desc(self):
        """ctypes struct kgcn_csr_batch pointing at the device arrays."""
        if self._desc is None:
            self._desc = _lib.CsrBatch(self.num_graphs, self.rows, self.cols, self.max_nnz,
                                       self.row_pad, 0, self.nnz, self.rowptr.data_ptr(),
                                       self.cv.data_ptr() if self.nnz else 0,
                                       self.slots.data_ptr() if self.slots is not None else 0,
                                       self.graph_ptr.data_ptr() if self.graph_ptr is not None else 0,
                                       self.block_ptr.data_ptr() if self.block_ptr is not None else 0,
                                       int(self.block_ptr.numel()) - 1 if self.block_ptr is not None else 0,
                                       self.block_rows_max if self.block_ptr is not None else 0)
        return self._desc

    def algorithmic_bytes(self):
        """CSR bytes of SURVEY 8d: 4(N+1) + 8 nnz per graph-channel."""
        return 4 * (self.num_graphs * (self.rows + 1)) + 8 * self.nnz


class CompactCSR:
    """The compact row-padded layout of a row-padded BatchedCSR (BatchedCSR.compact4()); rowptr and graph_ptr are the
    source's, `cv` holds the column words and, unless unit_values, the value stream."""

    def __init__(self, src, cv, slots, unit_values):
        self.src = src                  # the row-padded container (owns rowptr / graph_ptr)
        self.cv = cv                    # int32 [kgcn_compact_cv_words(nnz, not unit_values)]
        self.slots = slots              # int16 [T*M]
        self.unit_values = bool(unit_values)
        self.num_graphs, self.rows, self.cols = src.num_graphs, src.rows, src.cols
        self.max_nnz, self.nnz = src.max_nnz, src.nnz
        self._desc = None

    @classmethod
    def build(cls, p4):
        """kgcn_csr_compact4 on a row-padded container; None when a row does not fit the 16-bit slot."""
        import torch
        lib = _lib.lib
        T, M, dev = p4.num_graphs, p4.rows, p4.rowptr.device
        words = max(1, int(lib.kgcn_compact_cv_words(p4.nnz, 1)))
        cv = torch.zeros(words, device=dev, dtype=torch.int32)
        slots = torch.empty(max(1, T * M), device=dev, dtype=torch.int16)
        stats = torch.empty(2, device=dev, dtype=torch.int32)
        _lib.check(lib.kgcn_csr_compact4(p4.desc(), cv.data_ptr(), 1, slots.data_ptr(), _lib.ptr(stats),
                                         _lib.current_stream()), "kgcn_csr_compact4")
        non_unit, bad = (int(x) for x in stats.tolist())
        if bad:
            return None
        if non_unit == 0:                                   # no value stream: the column words alone
            cv = cv[:max(1, p4.nnz // 4)].clone()
        return cls(p4, cv, slots, non_unit == 0)

    def desc(self):
        """ctypes struct kgcn_csr_batch of the compact layout."""
        if self._desc is None:
            self._desc = _lib.CsrBatch(self.num_graphs, self.rows, self.cols, self.max_nnz,
                                       BatchedCSR.ROW_PAD_COMPACT, BatchedCSR.UNIT_VALUES if self.unit_values else 0,
                                       self.nnz, self.src.rowptr.data_ptr(), self.cv.data_ptr() if self.nnz else 0,
                                       self.slots.data_ptr() if self.src.slots is not None else 0,
                                       self.src.graph_ptr.data_ptr() if self.src.graph_ptr is not None else 0,
                                       0, 0, 0)
        return self._desc


class BatchedAdjacency:
    """All adjacency channels of a batch: what GraphConv / GINAggregate receive as `adj`.

    Built from the reference's list-of-lists adjs[b][ch] (kgcn/default_model.py:10,
    kgcn/feed.py:112-126) or from per-channel BatchedCSR objects."""

    def __init__(self, channels):
        if not channels:
            raise ValueError("at least one adjacency channel is required")
        t, m, k = channels[0].num_graphs, channels[0].rows, channels[0].cols
        for c in channels:
            if (c.num_graphs, c.rows, c.cols) != (t, m, k):
                raise ValueError("adjacency channels disagree on the batch shape")
        self.channels = list(channels)
        self._desc_arr = None
        self._desc_arr_t = None
        self.values = None      # see with_values()

    def with_values(self, values):
        """Same containers, with the adjacency VALUES as differentiable inputs: values[c] is a device
        fp32 tensor [nnz_c] in the CSR order of channel c (channels[c].values gives the stored ones).
        GraphConv then takes the differentiable route (per-channel Bspmm with d values, kgcn/
        bspmm_call.py:50-55) -- what the integrated-gradients loop of kgcn/visualization.py:187-260
        differentiates with respect to."""
        if len(values) != len(self.channels):
            raise ValueError("one value tensor per adjacency channel is required")
        out = BatchedAdjacency(self.channels)
        out.values = list(values)
        return out

    @classmethod
    def from_device_coo(cls, channels, num_graphs, n_nodes):
        """channels: one (graph, row, col, val) tuple of device tensors per adjacency channel (see
        BatchedCSR.from_device_coo) -- the whole batch packed on the GPU."""
        return cls([BatchedCSR.from_device_coo(g, r, c, v, num_graphs, n_nodes, n_nodes) for g, r, c, v in channels])

    @classmethod
    def from_adjs(cls, adjs, n_nodes=None, device="cuda", _flats=None):
        B = len(adjs)
        if B == 0:
            raise ValueError("empty batch")
        C = len(adjs[0])
        per_ch = [[adjs[b][ch] for b in range(B)] for ch in range(C)]
        flats = _flats if _flats is not None else [flatten_coo_list(m, need_shape=n_nodes is None) for m in per_ch]
        chans = [BatchedCSR.from_coo_list(per_ch[ch], rows=n_nodes, cols=n_nodes, device=device, _flat=flats[ch])
                 for ch in range(C)]
        # channels of one batch share the padded size
        M = max(c.rows for c in chans)
        K = max(c.cols for c in chans)
        if any(c.rows != M or c.cols != K for c in chans):
            chans = [BatchedCSR.from_coo_list(per_ch[ch], rows=M, cols=K, device=device, _flat=flats[ch]) for ch in range(C)]
        return cls(chans)

    @property
    def num_graphs(self):
        return self.channels[0].num_graphs

    @property
    def n_nodes(self):
        return self.channels[0].rows

    @property
    def num_channels(self):
        return len(self.channels)

    def desc_array(self, transposed=False):
        """Host array of kgcn_csr_batch descriptors (one per channel) for kgcn_bconv_f32 etc."""
        attr = "_desc_arr_t" if transposed else "_desc_arr"
        arr = getattr(self, attr)
        if arr is None:
            arr = (_lib.CsrBatch * len(self.channels))()
            for i, c in enumerate(self.channels):
                src = c.transpose() if transposed else c
                d = src.desc()
                ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(d), ctypes.sizeof(_lib.CsrBatch))
            setattr(self, attr, arr)
        return arr


class PackedAdjacencyCache:
    """Explicit, bounded cache of packed adjacency batches for callers that feed the reference's list-of-lists
    adjs[b][ch] (kgcn/feed.py:112-126 builds a fresh list of the SAME arrays every step, kgcn/core.py:267-269 feeds it).

    Keyed on CONTENT, not identity: a 128-bit digest of every index and value array (plus shapes), so mutating an entry in place
    -- which the reference's align_size / split_adj / normalize_adj all do -- yields a different key and a fresh pack.
    LRU of `max_entries` batches (device memory is held only for those); invalidate() drops everything.  The module
    instance `pack_cache` is what layers use for list inputs; set `kgcn_amd.batched_csr.pack_cache = None` to pack on
    every call, or hold a BatchedAdjacency yourself (BatchedAdjacency.from_adjs) and pass that -- no lookup at all."""

    def __init__(self, max_entries=8):
        import collections
        self.max_entries = int(max_entries)
        self._d = collections.OrderedDict()
        self.hits = self.misses = 0

    @staticmethod
    def _digest():
        try:
            import xxhash                              # 128-bit XXH3: ~10 GB/s (5 MB of triples in half a millisecond)
            return xxhash.xxh3_128()
        except ImportError:                            # pragma: no cover -- any 128-bit digest serves
            import hashlib
            return hashlib.blake2b(digest_size=16)

    @classmethod
    def fingerprint(cls, adj, n_nodes, device, _flats=None):
        """128-bit digest of every index / value byte and the per-graph entry counts, taken over the FLATTENED channels
        (two concatenated arrays per channel -- no per-matrix hashing loop); a CRC32 here would let two different batches
        of one shape collide once in ~2^32 and silently reuse the wrong CSR.  Returns (key, flats)."""
        B = len(adj)
        C = len(adj[0]) if B else 0
        for row in (adj[0], adj[-1]) if B else ():
            for m in row:
                v = _as_triple(m)[1]
                if hasattr(v, "requires_grad") and v.requires_grad:
                    return None, None                   # differentiable values: never cached
        flats = _flats if _flats is not None else \
            [flatten_coo_list([adj[b][ch] for b in range(B)], need_shape=n_nodes is None) for ch in range(C)]
        h = cls._digest()
        for idx, val, counts, M, K in flats:
            h.update(np.ascontiguousarray(idx).view(np.uint8).reshape(-1))
            h.update(np.ascontiguousarray(val).view(np.uint8).reshape(-1))
            h.update(counts.view(np.uint8))
            h.update(np.asarray([M, K, idx.dtype.num, val.dtype.num], np.int64).view(np.uint8))
        return (h.digest(), B, C, n_nodes, str(device)), flats

    def get(self, adj, n_nodes=None, device="cuda"):
        key, flats = self.fingerprint(adj, n_nodes, device)
        if key is not None and key in self._d:
            self._d.move_to_end(key)
            self.hits += 1
            return self._d[key]
        packed = BatchedAdjacency.from_adjs(adj, n_nodes=n_nodes, device=device, _flats=flats)
        self.misses += 1
        if key is not None and self.max_entries > 0:
            self._d[key] = packed
            while len(self._d) > self.max_entries:
                self._d.popitem(last=False)
        return packed

    def invalidate(self):
        self._d.clear()

    def __len__(self):
        return len(self._d)


pack_cache = PackedAdjacencyCache()


def as_batched_adjacency(adj, n_nodes=None, device="cuda"):
    """Accept a BatchedAdjacency, a BatchedCSR (single channel) or the reference's adjs[b][ch] list-of-lists (packed
    through `pack_cache`, a content-keyed LRU -- see PackedAdjacencyCache)."""
    if isinstance(adj, BatchedAdjacency):
        return adj
    if isinstance(adj, BatchedCSR):
        return BatchedAdjacency([adj])
    if hasattr(adj, "graph_ptr") and hasattr(adj, "adjacency"):        # kgcn_amd.ragged.RaggedBatch: its block-diagonal form
        return adj.adjacency
    if pack_cache is None:
        return BatchedAdjacency.from_adjs(adj, n_nodes=n_nodes, device=device)
    return pack_cache.get(adj, n_nodes=n_nodes, device=device)
