"""Host-side driver of the seeded Monte-Carlo PSF fit (include/fsq_montecarlo.h): the reference's fit_type='monte_carlo'
(pflib.py:117-177, 441-477) on the GPU under this library's explicit Philox draws.  PyTorch is used for device memory and
streams only; pflib routes fit_type='monte_carlo' with a seed here.  There is no CPU fallback (_host_montecarlo is the twin the
tests compare against)."""
import ctypes

import numpy as np

from . import _host_montecarlo as HT
from . import _native as N
from . import _native_montecarlo as NM
from . import engine as _engine


def check_args(n_iter, seed, first_field=0, n_fields=0):
    """ValueError for what the C ABI answers with FSQ_EINVAL."""
    HT.check_args(n_iter, seed)
    if not (0 <= int(first_field) and int(first_field) + int(n_fields) <= 1 << 32):
        raise ValueError("first_field + the number of fields must be in 0 .. 2^32")


def fit_rois(rois, ids=None, n_iter=1000, seed=0):
    """fsq_mc_fit_rois on float ROIs [n, 25] (or [n, 5, 5]) with ids uint32 [n, 2] = (pixel, field), zeros by default ->
    dict(rows FsqRow[n], fit float64 [n, 25], rms float64 [n], status int32 [n]) as NumPy arrays."""
    torch = _engine._torch()
    check_args(n_iter, seed)
    r = np.ascontiguousarray(rois, dtype=np.float64).reshape(-1, 25)
    n = len(r)
    i = np.zeros((n, 2), np.uint32) if ids is None else np.ascontiguousarray(ids, dtype=np.uint32).reshape(n, 2)
    dev = torch.device("cuda:%d" % torch.cuda.current_device())
    d_r = torch.from_numpy(r).to(dev)
    d_i = torch.from_numpy(i.view(np.int32)).to(dev)
    out = {"rows": torch.empty((n, 128), dtype=torch.uint8, device=dev), "fit": torch.empty((n, 25), dtype=torch.float64, device=dev),
           "rms": torch.empty(n, dtype=torch.float64, device=dev), "status": torch.empty(n, dtype=torch.int32, device=dev)}
    _engine.launch(NM.lib().fsq_mc_fit_rois, "fsq_mc_fit_rois", dev, d_r.data_ptr(), d_i.data_ptr(), n, int(n_iter), int(seed),
                   out["rows"].data_ptr(), out["fit"].data_ptr(), out["rms"].data_ptr(), out["status"].data_ptr())
    host = _engine.to_host(out)
    host["rows"] = host["rows"].view(N.ROW_DTYPE).reshape(-1)
    return host


def fit_candidates(images, cand, n_iter=1000, seed=0, first_field=0):
    """fsq_mc_fit_candidates on a uint16 stack [n_fields, H, W] and candidates int32 [n, 3] = (field, h, w) -> as fit_rois."""
    torch = _engine._torch()
    imgs = _engine.as_u16_fields(images)
    if imgs.ndim != 3:
        raise ValueError("images must have shape (n, H, W)")
    check_args(n_iter, seed, first_field, len(imgs))
    c = np.ascontiguousarray(cand, dtype=np.int32).reshape(-1, 3)
    n = len(c)
    dev = torch.device("cuda:%d" % torch.cuda.current_device())
    d_img = _engine.to_device_u16(imgs, dev)
    d_c = torch.from_numpy(c).to(dev)
    out = {"rows": torch.empty((n, 128), dtype=torch.uint8, device=dev), "fit": torch.empty((n, 25), dtype=torch.float64, device=dev),
           "rms": torch.empty(n, dtype=torch.float64, device=dev), "status": torch.empty(n, dtype=torch.int32, device=dev)}
    _engine.launch(NM.lib().fsq_mc_fit_candidates, "fsq_mc_fit_candidates", dev, d_img.data_ptr(), imgs.shape[0], imgs.shape[1],
                   imgs.shape[2], d_c.data_ptr(), n, int(n_iter), int(seed), int(first_field), out["rows"].data_ptr(),
                   out["fit"].data_ptr(), out["rms"].data_ptr(), out["status"].data_ptr())
    host = _engine.to_host(out)
    host["rows"] = host["rows"].view(N.ROW_DTYPE).reshape(-1)
    return host


class McPathRunner:
    """fsq_find_peptides_mc - detect -> Monte-Carlo fit -> consolidate -> peak records of a batch of same-shaped fields as one
    library call on the current stream, with its own workspace (engine.PathRunner's sibling).  Buffers grow on demand."""

    def __init__(self, n_fields, H, W, device=None, cand_cap=None, record_cap=None):
        torch = _engine._torch()
        self.torch = torch
        self.dev = torch.device(device or ("cuda:%d" % torch.cuda.current_device()))
        self.L = NM.lib()
        self.n_fields, self.H, self.W = int(n_fields), int(H), int(W)
        self.offsets = torch.zeros(self.n_fields + 1, dtype=torch.int32, device=self.dev)
        self.nkeep = torch.zeros(self.n_fields + 1, dtype=torch.int32, device=self.dev)
        self.status = torch.zeros(self.n_fields, dtype=torch.int32, device=self.dev)
        self._size(int(cand_cap or self.n_fields * max(1024, self.H * self.W // 48)),
                   int(record_cap or self.n_fields * max(256, self.H * self.W // 400)))

    def _size(self, cand_cap, record_cap):
        torch = self.torch
        self.cand_cap, self.record_cap = int(cand_cap), int(record_cap)
        nbytes = self.L.fsq_find_peptides_mc_workspace_bytes(self.n_fields, self.H, self.W, self.cand_cap, self.record_cap)
        if nbytes < 0:
            raise ValueError("invalid batch shape")
        self.ws = None
        self.records = None
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        self.records = torch.empty((self.record_cap, _engine.PEAK_RECORD_BYTES), dtype=torch.uint8, device=self.dev)

    def run(self, d_img, prm, r2_threshold=0.7, radius=4, n_iter=1000, seed=0, first_field=0, py2_round=True):
        """-> (records uint8[k, PEAK_RECORD_BYTES] - a view of this runner's buffer, valid until its next run -, offsets
        int32[n + 1], nkeep int32[n + 1], field status int32[n], candidates) on the device."""
        ncand, nrec = ctypes.c_int64(0), ctypes.c_int64(0)
        n_fields = int(d_img.shape[0])
        if not (1 <= n_fields <= self.n_fields) or tuple(d_img.shape[1:]) != (self.H, self.W) or d_img.element_size() != 2:
            raise ValueError("d_img must hold 1 .. %d fields of %d x %d 16-bit pixels" % (self.n_fields, self.H, self.W))
        while True:
            rc = self.L.fsq_find_peptides_mc(d_img.data_ptr(), n_fields, self.H, self.W, ctypes.byref(prm), float(r2_threshold),
                                             int(radius), 1 if py2_round else 0, int(n_iter), int(seed), int(first_field),
                                             self.cand_cap, self.records.data_ptr(), self.record_cap, self.offsets.data_ptr(),
                                             self.nkeep.data_ptr(), self.status.data_ptr(), ctypes.byref(ncand), ctypes.byref(nrec),
                                             self.ws.data_ptr(), self.ws.numel(), self.torch.cuda.current_stream(self.dev).cuda_stream)
            if rc != N.FSQ_ERANGE:
                break
            self._size(max(self.cand_cap, ncand.value + ncand.value // 8 + 1024), max(self.record_cap, nrec.value + nrec.value // 8 + 256))
        N.check(rc, "fsq_find_peptides_mc")
        return self.records[:nrec.value], self.offsets[:n_fields + 1], self.nkeep[:n_fields + 1], self.status[:n_fields], ncand.value


def encode_counts(nkeep, status):
    """One int32 per field for the record tables: peaks kept; -1 the re-key assertion (pflib.py:518) fired; -1 - s the field's
    first failing candidate had fit status s (-2: UnboundLocalError, -3: IndexError)."""
    nkeep, status = np.asarray(nkeep, np.int32), np.asarray(status, np.int32)
    return np.where(status != 0, -1 - status, nkeep).astype(np.int32)


def field_exception(f, count):
    """The exception the reference raises for a field whose count is negative."""
    if count == -1:
        return AssertionError("field %d: re-keyed peak collides with an existing key (pflib.py:518)" % f)
    if count == -1 - NM.MC_NO_MAXIMUM:
        return IndexError(HT.INDEX_ERROR_TEXT)
    if count == -1 - NM.MC_NEVER_IMPROVED:
        return UnboundLocalError(HT.UNBOUND_TEXT)
    raise ValueError("field %d: unknown count %d" % (f, count))


def find_peptides_stack(words, prm, r_2_threshold, radius, n_iter, seed, first_field, per, runner, py2_round=True, device=False):
    """find_peptides(fit_type='monte_carlo') over uint16 words [n, H, W]: a plain loop over chunks of `per` fields through
    fsq_find_peptides_mc (a fixed trip count per candidate has no tail for continuous batching to hide) ->
    (records uint8 [k, PEAK_RECORD_BYTES] of all fields in order, encode_counts int32 [n])."""
    torch = runner.torch
    n = len(words)
    check_args(n_iter, seed, first_field, n)
    recs, counts = [], []
    with torch.cuda.device(runner.dev):
        for a in range(0, n, per):
            part = words[a:a + per]
            d = _engine.to_device_u16(part, runner.dev)
            rec, offs, nk, st, _ = runner.run(d, prm, r_2_threshold, radius, n_iter, seed, first_field + a, py2_round)
            recs.append(rec.clone() if device else rec.cpu().numpy())
            counts.append(encode_counts(nk[:len(part)].cpu().numpy(), st.cpu().numpy()))
    counts = np.concatenate(counts) if counts else np.zeros(0, np.int32)
    if device:
        return (torch.cat(recs) if recs else torch.zeros((0, _engine.PEAK_RECORD_BYTES), dtype=torch.uint8, device=runner.dev)), counts
    return (np.concatenate(recs) if recs else np.zeros((0, _engine.PEAK_RECORD_BYTES), np.uint8)), counts


def float_sub_images(sub):
    """The sub_img of the reference's Monte-Carlo tuples from the integer ROIs int64 [k, 5, 5]: pflib.py:446-447's two numpy
    operations, (sub - min) / float(max)."""
    sub = np.asarray(sub, dtype=np.int64).reshape(-1, 5, 5)
    sub = sub - sub.min(axis=(1, 2), keepdims=True) if len(sub) else sub
    with np.errstate(all="ignore"):
        return sub / sub.max(axis=(1, 2), keepdims=True).astype(np.float64) if len(sub) else sub.astype(np.float64)
