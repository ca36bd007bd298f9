"""Thin handle around a KzScene* (the library's scene + device tables + device film; its camera, vertex data, materials, lights and mesh transforms can be edited in place)."""
import ctypes as C

import numpy as np

from . import abi

_TUNING_FIELDS = frozenset(name for name, _ in abi.KzTuning._fields_)


class Scene:
    """kz_scene_create -> [kz_scene_upload] -> kz_render* -> kz_film_download."""

    def __init__(self, desc, device=None, lib=None):
        self.lib = lib or abi.load_library()      # (lib: a development build of the library, abi.load_dev_library() - tests only)
        self.desc = desc
        self._base = {}                                      # mesh -> (V, N) base data of the meshes a transform has placed (set_transforms)
        cdesc = desc.to_c()
        h = C.c_void_p()
        abi.check(self.lib, self.lib.kz_scene_create(C.byref(cdesc), C.byref(h)))
        self.h = h
        self.device = None
        w, hh, b = C.c_int32(), C.c_int32(), C.c_int32()
        abi.check(self.lib, self.lib.kz_film_dims(self.h, C.byref(w), C.byref(hh), C.byref(b)))
        self.width, self.height, self.border = w.value, hh.value, b.value
        n = C.c_uint32()
        abi.check(self.lib, self.lib.kz_scene_sample_count(self.h, C.byref(n)))
        self.sample_count = n.value
        if device is not None:
            self.upload(device)

    def close(self):
        if getattr(self, "h", None):
            self.lib.kz_scene_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def bvh_info(self):
        info = abi.KzBvhInfo()
        abi.check(self.lib, self.lib.kz_scene_bvh_info(self.h, C.byref(info)))
        return {k: getattr(info, k) for k, _ in info._fields_}

    def set_camera(self, camera):
        """kz_scene_set_camera (include/kazen_mi355x_edit.h): `camera` holds keys of SceneDescription.camera; the others keep their values.
        width, height and rfilter must stay the scene's. Scene.desc.camera follows."""
        from .scenes import camera_to_c
        cam = dict(self.desc.camera)
        cam.update(camera)
        if "toWorld" in camera:
            cam["toWorld"] = np.array(camera["toWorld"], np.float32)
        c = camera_to_c(cam, abi.KzCamera())
        abi.check(self.lib, self.lib.kz_scene_set_camera(self.h, C.byref(c)))
        self.desc.camera = cam

    def set_vertices(self, updates):
        """kz_scene_set_vertices (include/kazen_mi355x_edit.h) for a batch {mesh: V} or {mesh: (V, N)}: V / N (nV, 3) float32 from host memory, N exactly when
        the mesh has normals. Scene.desc's meshes follow (new arrays: the old ones are not written)."""
        rows, keep = [], []
        for m, x in updates.items():
            V, N = (x if isinstance(x, tuple) else (x, None))
            V = np.ascontiguousarray(V, np.float32).reshape(-1, 3)
            N = None if N is None else np.ascontiguousarray(N, np.float32).reshape(-1, 3)
            keep.append((int(m), V, N))
            rows.append(abi.KzVertexUpdate(int(m) if int(m) >= 0 else 0xFFFFFFFF, V.shape[0], V.ctypes.data_as(abi.f32p), N.ctypes.data_as(abi.f32p) if N is not None else None))
        arr = (abi.KzVertexUpdate * max(1, len(rows)))(*rows)
        abi.check(self.lib, self.lib.kz_scene_set_vertices(self.h, arr, len(rows)))
        for m, V, N in keep:
            self.desc.meshes[m] = dict(self.desc.meshes[m], V=V.copy(), N=None if N is None else N.copy())
            self._base.pop(m, None)                          # new base data: the mesh's transform is gone

    def set_bsdfs(self, updates):
        """kz_scene_set_bsdfs (include/kazen_mi355x_edit.h) for {mesh: bsdf dict}: the edited description is flattened as kz_scene_create's input is and the BSDF rows
        that differ are sent. ValueError unless the texture and image tables, the mesh -> row assignment and the row count come out as before (create a new scene
        for those). Scene.desc follows."""
        import copy
        old, new = copy.copy(self.desc), copy.copy(self.desc)
        new.meshes = list(self.desc.meshes)
        for m, b in updates.items():
            if new.meshes[int(m)]["bsdf"] is None or b is None:
                raise ValueError("mesh %d: a mesh without a BSDF keeps the default row, and a mesh with one keeps a row: create a new scene" % int(m))
            new.meshes[int(m)] = dict(new.meshes[int(m)], bsdf=b)
        co = old.to_c()
        new._tex_seed = old._tex_list                        # the scene's textures keep their ids; a texture it does not have would be appended (refused below)
        cn = new.to_c()
        io, im = old._keep[-1], new._keep[-1]
        same = (co.nBsdfs == cn.nBsdfs and co.nTextures == cn.nTextures and co.nImages == cn.nImages
                and all(co.meshes[i].bsdf == cn.meshes[i].bsdf for i in range(co.nMeshes))
                and all(bytes(co.textures[i]) == bytes(cn.textures[i]) for i in range(co.nTextures))
                and all(a is b or (a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)) for a, b in zip(io, im)))
        if not same:
            raise ValueError("set_bsdfs: the edit changes the texture table, the image table, the mesh -> row assignment or the row count: create a new scene")
        rows = [abi.KzBsdfUpdate(i, cn.bsdfs[i]) for i in range(cn.nBsdfs) if bytes(co.bsdfs[i]) != bytes(cn.bsdfs[i])]
        arr = (abi.KzBsdfUpdate * max(1, len(rows)))(*rows)
        abi.check(self.lib, self.lib.kz_scene_set_bsdfs(self.h, arr, len(rows)))
        self.desc.meshes, self.desc._tex_seed = new.meshes, new._tex_seed

    def set_lights(self, updates):
        """kz_scene_set_lights for {mesh: light dict (scenes.area)}: colour, intensity and lightPrimaryVisibility of meshes that emit already. Scene.desc follows."""
        lights = [i for i, m in enumerate(self.desc.meshes) if m["light"] is not None]
        rows = []
        for m, l in updates.items():
            if int(m) not in lights or l is None:
                raise ValueError("mesh %d: which meshes emit does not change: create a new scene" % int(m))
            k = abi.KzLight()
            k.color[:] = l["color"]
            k.intensity = l["intensity"]
            k.primaryVisibility = 1 if l["lightPrimaryVisibility"] else 0
            rows.append(abi.KzLightUpdate(lights.index(int(m)), k))
        arr = (abi.KzLightUpdate * max(1, len(rows)))(*rows)
        abi.check(self.lib, self.lib.kz_scene_set_lights(self.h, arr, len(rows)))
        meshes = list(self.desc.meshes)
        for m, l in updates.items():
            meshes[int(m)] = dict(meshes[int(m)], light=dict(l))
        self.desc.meshes = meshes

    def set_transforms(self, updates):
        """kz_scene_set_transforms for {mesh: 4x4 (row-major, as camera toWorld)}: the mesh's BASE data (its V / N at creation or from its last set_vertices) under
        the matrix; transforms of one mesh do not compose. Scene.desc holds the transformed arrays afterwards (scenes.transform_vertices states the arithmetic)."""
        from .scenes import transform_vertices
        rows, mats = [], {}
        for m, M in updates.items():
            M = np.ascontiguousarray(M, np.float32).reshape(4, 4)
            mats[int(m)] = M
            k = abi.KzTransformUpdate()
            k.mesh = int(m) if int(m) >= 0 else 0xFFFFFFFF
            k.toWorld[:] = M.reshape(16).tolist()
            rows.append(k)
        arr = (abi.KzTransformUpdate * max(1, len(rows)))(*rows)
        abi.check(self.lib, self.lib.kz_scene_set_transforms(self.h, arr, len(rows)))
        meshes = list(self.desc.meshes)
        for m, M in mats.items():
            if m not in self._base:
                self._base[m] = (meshes[m]["V"], meshes[m]["N"])
            V, N = transform_vertices(M, *self._base[m])
            meshes[m] = dict(meshes[m], V=V, N=N)
        self.desc.meshes = meshes

    def table(self, table, device=-1):
        """kz_scene_table: a flat table of the scene as raw bytes (numpy uint8): device -1 = the host copy, else that replica's (abi.KZ_TABLE_*)."""
        n = C.c_size_t()
        abi.check(self.lib, self.lib.kz_scene_table(self.h, int(device), int(table), None, 0, C.byref(n)))
        out = np.zeros(n.value, np.uint8)
        abi.check(self.lib, self.lib.kz_scene_table(self.h, int(device), int(table), out.ctypes.data_as(C.c_void_p), out.size, C.byref(n)))
        return out

    def upload(self, device=0):
        """Adds a replica on `device` (the first one uploaded is the primary, which the calls without a device address)."""
        abi.check(self.lib, self.lib.kz_scene_upload(self.h, int(device)))
        if self.device is None:
            self.device = int(device)

    def evict(self, device=-1):
        abi.check(self.lib, self.lib.kz_scene_evict(self.h, int(device)))
        if device < 0 or device == self.device:
            left = self.devices()
            self.device = left[0] if left else None            # the next replica becomes the one the calls without a device address

    def devices(self):
        buf = (C.c_int32 * 64)()
        n = C.c_uint32()
        abi.check(self.lib, self.lib.kz_scene_devices(self.h, buf, 64, C.byref(n)))
        return [int(buf[i]) for i in range(n.value)]

    def _opts(self, sample_begin=0, sample_end=0, tiles=None, accumulate=False, pipeline=0, stream=None, device=None,
              passes_in_flight=0, pass_items=0, max_state_bytes=0, tune=None, tile_dealing=0, shadow_beside=0, pass_halves=0):
        o = abi.KzRenderOpts()
        o.sampleBegin, o.sampleEnd = sample_begin, sample_end
        keep = None
        if tiles is not None:
            keep = (abi.KzTile * len(tiles))(*[abi.KzTile(*t) for t in tiles])
            o.tiles, o.nTiles = keep, len(tiles)
        o.pipeline = pipeline
        o.accumulate = 1 if accumulate else 0
        o.stream = stream
        o.device = (self.device or 0) if device is None else int(device)
        o.passesInFlight, o.passItems, o.maxStateBytes = int(passes_in_flight), int(pass_items), int(max_state_bytes)
        o.tileDealing = int(tile_dealing)
        o.shadowBeside = int(shadow_beside)
        o.passHalves = int(pass_halves)
        for k, v in (tune or {}).items():
            # a name KzTuning does not have is refused, not dropped: ctypes would keep it as a plain attribute the library never sees (a typo, or
            # one of the names the reserved dev0 .. dev5 words had - bvh2, ... - whose values the library refuses)
            if k not in _TUNING_FIELDS:
                raise abi.KzError(abi.KZ_ERR_UNSUPPORTED, "KzTuning has no field %r (its fields: %s)" % (k, ", ".join(sorted(_TUNING_FIELDS))))
            setattr(o.tune, k, int(v))
        return o, keep

    def render(self, sample_begin=0, sample_end=0, tiles=None, accumulate=False, pipeline=0, stream=None, **kw):
        """kz_render. Keywords: device, passes_in_flight, pass_items, max_state_bytes, shadow_beside, pass_halves, tune={KzTuning field: value}."""
        o, keep = self._opts(sample_begin, sample_end, tiles, accumulate, pipeline, stream, **kw)
        abi.check(self.lib, self.lib.kz_render(self.h, C.byref(o)))

    def render_tiles(self, tiles, device=None, sample_begin=0, sample_end=0, download=True, packed=False, **kw):
        """kz_render_tiles: blocking render of `tiles` on `device`. download=True returns that replica's whole film, packed=True the
        PACKED film rects of the tiles (1-D float32: every tile's (h+2b) x (w+2b) x 4 rect in list order), download=False nothing."""
        o, _ = self._opts(sample_begin, sample_end, **kw)
        arr = (abi.KzTile * len(tiles))(*[abi.KzTile(*t) for t in tiles])
        dev = (self.device or 0) if device is None else int(device)
        o.packedOutput = 1 if packed else 0
        out = np.empty(self.packed_floats(tiles), np.float32) if packed else self._film_out()[0] if download else None
        abi.check(self.lib, self.lib.kz_render_tiles(self.h, C.byref(o), arr, len(tiles), dev,
                                                      out.ctypes.data_as(abi.f32p) if out is not None else None, out.size if out is not None else 0))
        return out

    def render_dealt(self, tiles, counter, takers=1, batch_tiles=0, device=None, sample_begin=0, sample_end=0, **kw):
        """kz_render_tiles with a KzTileDealer: `tiles` is the WHOLE list every taker passes, `counter` a numpy uint32 array of one element that all
        takers share (process-local, or a np.memmap of a file in /dev/shm for the ranks of a node; zeroed by the launcher). Renders the batches this
        call wins and returns the tiles it took, in the order it took them (hand them to film_tiles for the gather)."""
        o, _ = self._opts(sample_begin, sample_end, **kw)
        arr = (abi.KzTile * len(tiles))(*[abi.KzTile(*t) for t in tiles])
        dev = (self.device or 0) if device is None else int(device)
        taken = np.zeros(2 * len(tiles) + 2, np.uint32)
        n_taken = np.zeros(1, np.uint32)
        assert counter.dtype == np.uint32 and counter.size >= 1
        # (a counter array of two or more words: word 1 is the takers' agreement word, KzTileDealer.agreed)
        agreed = C.cast(counter.ctypes.data + 4, abi.u32p) if counter.size >= 2 else None
        dl = abi.KzTileDealer(counter.ctypes.data_as(abi.u32p), int(batch_tiles), int(takers), taken.ctypes.data_as(abi.u32p), taken.size, n_taken.ctypes.data_as(abi.u32p), agreed)
        o.dealer = C.pointer(dl)
        abi.check(self.lib, self.lib.kz_render_tiles(self.h, C.byref(o), arr, len(tiles), dev, None, 0))
        out = []
        for k in range(0, int(n_taken[0]), 2):
            out += list(tiles[int(taken[k]):int(taken[k + 1])])
        return out

    def packed_floats(self, tiles):
        arr = (abi.KzTile * len(tiles))(*[abi.KzTile(*t) for t in tiles])
        n = C.c_size_t()
        abi.check(self.lib, self.lib.kz_tiles_packed_floats(self.h, arr, len(tiles), C.byref(n)))
        return int(n.value)

    def film_tiles(self, tiles, device=None):
        """kz_film_download_tiles: the packed film rects of `tiles` from the replica's film."""
        arr = (abi.KzTile * len(tiles))(*[abi.KzTile(*t) for t in tiles])
        dev = (self.device or 0) if device is None else int(device)
        out = np.empty(self.packed_floats(tiles), np.float32)
        abi.check(self.lib, self.lib.kz_film_download_tiles(self.h, dev, arr, len(tiles), out.ctypes.data_as(abi.f32p), out.size))
        return out

    def merge_tiles(self, film, tiles, packed, threads=0):
        """kz_film_merge_tiles: film += the packed rects, in list order (ImageBlock::put(ImageBlock&), block.cpp:87-96)."""
        arr = (abi.KzTile * len(tiles))(*[abi.KzTile(*t) for t in tiles])
        packed = np.ascontiguousarray(packed, np.float32)
        assert film.dtype == np.float32 and film.flags["C_CONTIGUOUS"]
        abi.check(self.lib, self.lib.kz_film_merge_tiles(film.ctypes.data_as(abi.f32p), self.width, self.height, self.border, arr, len(tiles),
                                                          packed.ctypes.data_as(abi.f32p), packed.size, int(threads)))
        return film

    def merge_rects(self, film, entries, threads=0):
        """kz_film_merge_rects: entries = [(tile, float32 array holding that tile's packed rect)], added to `film` in list order (row-major tile order = the
        film every other path gives). The arrays may be views into different buffers: nothing is copied."""
        n = len(entries)
        arr = (abi.KzTile * n)(*[abi.KzTile(*t) for t, _ in entries])
        ptrs = (abi.f32p * n)(*[C.cast(r.ctypes.data, abi.f32p) for _, r in entries])
        b = self.border
        for t, r in entries:
            if r.dtype != np.float32 or r.size != (t[2] + 2 * b) * (t[3] + 2 * b) * 4 or not r.flags["C_CONTIGUOUS"]:
                raise ValueError("merge_rects: the rect of tile %s must be %d contiguous float32" % (t, (t[2] + 2 * b) * (t[3] + 2 * b) * 4))
        abi.check(self.lib, self.lib.kz_film_merge_rects(film.ctypes.data_as(abi.f32p), self.width, self.height, self.border, arr, ptrs, n, int(threads)))
        return film

    def _film_shape(self):
        return (self.height + 2 * self.border, self.width + 2 * self.border, 4)       # the frame with its filter apron, (rgb * w, w) per texel

    def empty_film(self):
        return np.zeros(self._film_shape(), np.float32)

    def _film_out(self):
        """An uninitialised film for a download to fill: (the array, its float pointer, its number of floats)."""
        out = np.empty(self._film_shape(), np.float32)
        return out, out.ctypes.data_as(abi.f32p), out.size

    def render_multi(self, devices, tile_size=0, sample_begin=0, sample_end=0, **kw):
        """kz_render_multi: one host thread per device, tiles dealt by area, films summed on the host in device order.
        Returns (film, per-device ms)."""
        o, _ = self._opts(sample_begin, sample_end, **kw)
        devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        out, ptr, n = self._film_out()
        ms = np.zeros(len(devices), np.float32)
        abi.check(self.lib, self.lib.kz_render_multi(self.h, C.byref(o), devs, len(devices), int(tile_size), ptr, n,
                                                      ms.ctypes.data_as(abi.f32p)))
        if self.device is None:
            self.device = int(devices[0])
        return out, ms

    def last_pass_info(self):
        info = abi.KzPassInfo()
        abi.check(self.lib, self.lib.kz_last_pass_info(self.h, C.byref(info)))
        return info.as_dict()

    def pass_mode_info(self, device=-1):
        """kz_pass_mode_info: what the replica measured about its large passes and what it keeps (None while undecided)."""
        m = abi.KzPassModeInfo()
        abi.check(self.lib, self.lib.kz_pass_mode_info(self.h, int(device), C.byref(m)))
        d = {"kept": (None, "one stream", "shadow rays beside", "halves")[m.kept + 1], "timed_passes": int(m.timedPasses), "items": int(m.items)}
        if m.kept >= 0:
            d.update({"ms_one_stream": [round(float(m.msOneStream[0]), 2), round(float(m.msOneStream[1]), 2)], "ms_shadow_beside": round(float(m.msShadowBeside), 2), "ms_halves": round(float(m.msHalves), 2)})
        return d

    def last_grow_note(self):
        """Why the pass context of the last render stopped growing short of its target ('' if it did not)."""
        buf = C.create_string_buffer(512)
        abi.check(self.lib, self.lib.kz_last_grow_note(self.h, buf, 512))
        return buf.value.decode()

    def sync(self):
        abi.check(self.lib, self.lib.kz_sync(self.h))

    def film(self):
        out, ptr, n = self._film_out()
        abi.check(self.lib, self.lib.kz_film_download(self.h, ptr, n))
        return out

    def film_clear(self, stream=None):
        abi.check(self.lib, self.lib.kz_film_clear(self.h, stream))

    def rgb(self, film=None):
        film = self.film() if film is None else np.ascontiguousarray(film, np.float32)
        out = np.empty((self.height, self.width, 3), np.float32)
        abi.check(self.lib, self.lib.kz_film_to_rgb(film.ctypes.data_as(abi.f32p), self.width, self.height, self.border,
                                                     out.ctypes.data_as(abi.f32p)))
        return out

    def trace_rays(self, o, d, tmin, tmax):
        o = np.ascontiguousarray(o, np.float32)
        d = np.ascontiguousarray(d, np.float32)
        n = o.shape[0]
        tmin = np.ascontiguousarray(np.broadcast_to(np.asarray(tmin, np.float32), (n,)))
        tmax = np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, np.float32), (n,)))
        hits = (abi.KzHit * n)()
        abi.check(self.lib, self.lib.kz_trace_rays(self.h, n, o.ctypes.data_as(abi.f32p), d.ctypes.data_as(abi.f32p),
                                                   tmin.ctypes.data_as(abi.f32p), tmax.ctypes.data_as(abi.f32p), hits))
        return hits_to_arrays(hits, n)

    def trace_rays_wf(self, o, d, tmin, tmax, kernel=0, queue=None, pending=None, hits=None, sums=None, stats=False, refill=0, postpone=0, batch=0,
                      lds_stack=0, grid_blocks=0, packet_batch=0):
        """kz_trace_rays_wf (include/kazen_mi355x_dev.h): the traversal launches of a render - kernel 0 per-lane closest hit, 1 packet, 2 walk-through ray, 3 shadow
        test - on these rays, one per slot. hits: (n, 4) float32 = t, u, v and the bits of gid, the slots' records before the launch (default: NaN, NaN, NaN,
        0xFFFFFFFF); sums, pending: (n, 3). Returns {"t", "u", "v", "gid", "mesh", "prim", "sums", "info"}."""
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        n = o.shape[0]
        tmin = np.ascontiguousarray(np.broadcast_to(np.asarray(tmin, np.float32), (n,)))
        tmax = np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, np.float32), (n,)))
        rec = np.zeros(n, np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("gid", "<u4"), ("mesh", "<i4"), ("prim", "<i4")]))
        assert rec.itemsize == C.sizeof(abi.KzTraceWfHit)
        if hits is None:
            rec["t"] = rec["u"] = rec["v"] = np.nan
            rec["gid"] = 0xFFFFFFFF
        else:
            hits = np.ascontiguousarray(hits, np.float32).reshape(n, 4)
            rec["t"], rec["u"], rec["v"], rec["gid"] = hits[:, 0], hits[:, 1], hits[:, 2], hits[:, 3].view(np.uint32)
        sums = np.zeros((n, 3), np.float32) if sums is None else np.array(sums, np.float32).reshape(n, 3)
        pend = None if pending is None else np.ascontiguousarray(pending, np.float32).reshape(n, 3)
        q = None if queue is None else np.ascontiguousarray(queue, np.uint32).reshape(-1)
        opts = abi.KzTraceWfOpts(int(kernel), 1 if stats else 0, int(refill), int(postpone), int(batch), int(lds_stack), int(grid_blocks), int(packet_batch))
        info = abi.KzTraceWfInfo()
        abi.check(self.lib, self.lib.kz_trace_rays_wf(self.h, C.byref(opts), n, o.ctypes.data_as(abi.f32p), d.ctypes.data_as(abi.f32p), tmin.ctypes.data_as(abi.f32p),
                                                      tmax.ctypes.data_as(abi.f32p), None if q is None else q.ctypes.data_as(abi.u32p), 0 if q is None else q.size,
                                                      None if pend is None else pend.ctypes.data_as(abi.f32p), rec.ctypes.data_as(C.POINTER(abi.KzTraceWfHit)),
                                                      sums.ctypes.data_as(abi.f32p), C.byref(info)))
        out = {k: rec[k].copy() for k in rec.dtype.names}
        out["sums"], out["info"] = sums, info.as_dict()
        return out

    def render_samples(self, pxy, idx):
        pxy = np.ascontiguousarray(pxy, np.int32)
        idx = np.ascontiguousarray(idx, np.uint32)
        n = idx.shape[0]
        out = np.zeros((n, 5), np.float32)
        abi.check(self.lib, self.lib.kz_render_samples(self.h, n, pxy.ctypes.data_as(C.POINTER(C.c_int32)),
                                                       idx.ctypes.data_as(abi.u32p), out.ctypes.data_as(abi.f32p)))
        return out

    # ---- feature films beside the picture (include/kazen_mi355x_aov.h)
    @staticmethod
    def _aov_mask(names):
        if isinstance(names, int):
            return int(names)
        if isinstance(names, str):
            names = [names]
        mask = 0
        for n in names or ():
            if n not in abi.AOV_BITS:
                raise ValueError("unknown AOV %r (known: %s)" % (n, ", ".join(sorted(abi.AOV_BITS))))
            mask |= abi.AOV_BITS[n]
        return mask

    def set_aovs(self, names):
        """kz_scene_set_aovs: `names` = any of "albedo", "normal", "depth" (or the bit mask itself; () / 0 switches the feature films off). An AOV that is
        switched on covers the samples rendered from then on: clear the film when accumulating."""
        abi.check(self.lib, self.lib.kz_scene_set_aovs(self.h, self._aov_mask(names)))

    def aovs(self):
        m = C.c_uint32()
        abi.check(self.lib, self.lib.kz_scene_aovs(self.h, C.byref(m)))
        return [n for n, b in abi.AOV_BITS.items() if m.value & b]

    def aov_film(self, name, device=None):
        """kz_aov_download[_on]: the AOV's film, (h + 2b, w + 2b, 4) = (value * w, w) like film()."""
        out, ptr, n = self._film_out()
        if device is None:
            abi.check(self.lib, self.lib.kz_aov_download(self.h, self._aov_mask(name), ptr, n))
        else:
            abi.check(self.lib, self.lib.kz_aov_download_on(self.h, int(device), self._aov_mask(name), ptr, n))
        return out

    def aov(self, name, device=None):
        """The AOV's values, (h, w, 3): its film divided by the filter weight (kz_film_to_rgb); depth is replicated into the three channels."""
        return self.rgb(self.aov_film(name, device))

    def aov_info(self, device=-1):
        """kz_aov_info: bytes the AOV tap sums and films hold on that replica."""
        b = C.c_uint64()
        abi.check(self.lib, self.lib.kz_aov_info(self.h, int(device), C.byref(b)))
        return int(b.value)

    def aov_samples(self, pxy, idx):
        """kz_aov_samples: (n, 10) = sample x, y | albedo rgb | normal xyz | depth | hit, shaped like render_samples."""
        pxy = np.ascontiguousarray(pxy, np.int32)
        idx = np.ascontiguousarray(idx, np.uint32)
        n = idx.shape[0]
        out = np.zeros((n, 10), np.float32)
        abi.check(self.lib, self.lib.kz_aov_samples(self.h, n, pxy.ctypes.data_as(C.POINTER(C.c_int32)), idx.ctypes.data_as(abi.u32p), out.ctypes.data_as(abi.f32p)))
        return out

    # ---- ID mattes beside the picture (include_ext/kazen_mi355x_matte.h)
    @staticmethod
    def _matte_mask(names):
        if isinstance(names, int):
            return int(names)
        if isinstance(names, str):
            names = [names]
        mask = 0
        for n in names or ():
            if n not in abi.MATTE_BITS:
                raise ValueError("unknown matte key %r (known: %s)" % (n, ", ".join(sorted(abi.MATTE_BITS))))
            mask |= abi.MATTE_BITS[n]
        return mask

    def set_mattes(self, names):
        """kz_scene_set_mattes: `names` = any of "mesh", "bsdf" (or the bit mask itself; () / 0 switches the mattes off). A key that leaves the mask loses its
        tables; one that enters starts from zero."""
        abi.check(self.lib, self.lib.kz_scene_set_mattes(self.h, self._matte_mask(names)))

    def mattes(self):
        m = C.c_uint32()
        abi.check(self.lib, self.lib.kz_scene_mattes(self.h, C.byref(m)))
        return [n for n, b in abi.MATTE_BITS.items() if m.value & b]

    def matte(self, key, device=None):
        """kz_matte_download[_on]: the key's table, (h, w) records of abi.MATTE_DTYPE (id[7], count[7], other, miss), every record ranked: count descending,
        ties to the lower id, free slots last."""
        out = np.zeros((self.height, self.width), abi.MATTE_DTYPE)
        ptr = out.ctypes.data_as(C.POINTER(abi.KzMatteTexel))
        if device is None:
            abi.check(self.lib, self.lib.kz_matte_download(self.h, self._matte_mask(key), ptr, out.size))
        else:
            abi.check(self.lib, self.lib.kz_matte_download_on(self.h, int(device), self._matte_mask(key), ptr, out.size))
        return out

    def matte_layer(self, key, id, device=None):
        """kz_matte_layer: (h, w) float32, the coverage of `id`: its count over the pixel's samples (0 where it has no slot or the pixel no samples)."""
        out = np.zeros((self.height, self.width), np.float32)
        abi.check(self.lib, self.lib.kz_matte_layer(self.h, -1 if device is None else int(device), self._matte_mask(key), int(id), out.ctypes.data_as(abi.f32p), out.size))
        return out

    def matte_top(self, key, device=None):
        """kz_matte_top: (h, w) uint32, the id with the largest count of every pixel (abi.KZ_MATTE_NONE: the misses are at least as many, or no samples)."""
        out = np.zeros((self.height, self.width), np.uint32)
        abi.check(self.lib, self.lib.kz_matte_top(self.h, -1 if device is None else int(device), self._matte_mask(key), out.ctypes.data_as(abi.u32p), out.size))
        return out

    def matte_info(self, device=-1):
        """kz_matte_info: bytes the matte tables hold on that replica."""
        b = C.c_uint64()
        abi.check(self.lib, self.lib.kz_matte_info(self.h, int(device), C.byref(b)))
        return int(b.value)

    def matte_accumulate_items(self, keys, pix_list, tables=None, device=None, form=0):
        """kz_matte_accumulate_items, the test surface: the product kernel on the (nPix, S) key plane `keys` (abi.KZ_MATTE_NONE = a miss) of the pixels `pix_list`
        (x | y << 16), starting from the records `tables` (nPix of abi.MATTE_DTYPE; None: zeros). Returns the unranked records. form: 0 as a render picks,
        1 one lane per pixel, 2 one wave per pixel."""
        keys = np.ascontiguousarray(keys, np.uint32)
        pix_list = np.ascontiguousarray(pix_list, np.uint32)
        n_pix, S = keys.shape
        out = np.zeros(n_pix, abi.MATTE_DTYPE) if tables is None else np.ascontiguousarray(tables, abi.MATTE_DTYPE).copy()
        if out.shape != (n_pix,) or pix_list.shape != (n_pix,):
            raise ValueError("keys (nPix, S), pix_list (nPix,), tables (nPix,)")
        abi.check(self.lib, self.lib.kz_matte_accumulate_items(self.h, -1 if device is None else int(device), keys.ctypes.data_as(abi.u32p), n_pix, S,
                                                               pix_list.ctypes.data_as(abi.u32p), out.ctypes.data_as(C.POINTER(abi.KzMatteTexel)), int(form)))
        return out

    # ---- the picture denoised on the device, guided by its feature films (include/kazen_mi355x_denoise.h)
    def denoise(self, device=None, **opts):
        """kz_denoise[_on]: filters the replica's picture with the enabled feature films as guides; the result stays on the device (denoised_film,
        denoised_srgb8) until the next denoise. Options: see denoise_opts."""
        o = denoise_opts(**opts)
        if device is None:
            abi.check(self.lib, self.lib.kz_denoise(self.h, C.byref(o)))
        else:
            abi.check(self.lib, self.lib.kz_denoise_on(self.h, int(device), C.byref(o)))

    def denoised_film(self, device=None):
        """kz_denoise_download: (h + 2b, w + 2b, 4) = (rgb, 1) in the frame pixels that had samples, zeros elsewhere - rgb() and the writers of output.py take it like film()."""
        out, ptr, n = self._film_out()
        abi.check(self.lib, self.lib.kz_denoise_download(self.h, -1 if device is None else int(device), ptr, n))
        return out

    def denoised_srgb8(self, device=None):
        """kz_denoise_to_srgb8: (h, w, 3) uint8, the raster srgb8() makes of the film, of the denoised picture."""
        out = np.zeros((self.height, self.width, 3), np.uint8)
        abi.check(self.lib, self.lib.kz_denoise_to_srgb8(self.h, -1 if device is None else int(device), out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size))
        return out

    def denoise_info(self, device=-1):
        """kz_denoise_info: bytes the denoiser's buffers hold on that replica."""
        b = C.c_uint64()
        abi.check(self.lib, self.lib.kz_denoise_info(self.h, int(device), C.byref(b)))
        return int(b.value)

    def denoise_release(self, device=-1):
        abi.check(self.lib, self.lib.kz_denoise_release(self.h, int(device)))

    # ---- the second-moment film and the variance-guided denoiser (include/kazen_mi355x_variance.h)
    def set_variance(self, on=True):
        """kz_scene_set_variance: True / False (or a KZ_VARIANCE_* mode: 2 = two tap launches, 3 = the one-pass tap kernel - the same film either way). A film that is
        switched on covers the samples rendered from then on."""
        abi.check(self.lib, self.lib.kz_scene_set_variance(self.h, int(on)))

    def variance(self):
        m = C.c_int32()
        abi.check(self.lib, self.lib.kz_scene_variance(self.h, C.byref(m)))
        return int(m.value)

    def moment_film(self, device=None):
        """kz_variance_download: the second-moment film, (h + 2b, w + 2b, 4) = (w r^2, w g^2, w b^2, w) like film()."""
        out, ptr, n = self._film_out()
        abi.check(self.lib, self.lib.kz_variance_download(self.h, -1 if device is None else int(device), ptr, n))
        return out

    def variance_info(self, device=-1):
        """kz_variance_info: (bytes the film holds on that replica, samples per pixel it has been given since it was last zeroed)."""
        b, n = C.c_uint64(), C.c_uint32()
        abi.check(self.lib, self.lib.kz_variance_info(self.h, int(device), C.byref(b), C.byref(n)))
        return int(b.value), int(n.value)

    def denoise_variance(self, device=None, sigma_variance=0.0, samples=0, vflags=0, vreserved=0, **opts):
        """kz_denoise_variance: denoise() with a colour tolerance that follows the second-moment film's variance (sigma_color defaults to 2.0 here); the result is read
        like denoise()'s. Options: denoise_opts' and variance_opts'."""
        o, v = denoise_opts(**opts), variance_opts(sigma_variance, samples, vflags, vreserved)
        abi.check(self.lib, self.lib.kz_denoise_variance(self.h, -1 if device is None else int(device), C.byref(o), C.byref(v)))

    # ---- adaptive sampling (include_ext/kazen_mi355x_adaptive.h)
    def render_adaptive(self, threshold, floor=0.0, min_samples=0, max_samples=0, step=0, block=0, outlier_permille=0, aflags=0, **kw):
        """kz_render_adaptive: rounds of samples over the blocks whose relative standard error is still above `threshold` (set_variance(True) first). Blocks until the
        last round is tested. Keywords beyond the rule's: render()'s. Returns the KzAdaptiveInfo as a dict (rounds, blocks, converged, atCap, samples, bytes)."""
        o, keep = self._opts(**kw)
        a = adaptive_opts(threshold, floor, min_samples, max_samples, step, block, outlier_permille, aflags)
        info = abi.KzAdaptiveInfo()
        abi.check(self.lib, self.lib.kz_render_adaptive(self.h, C.byref(o), C.byref(a), C.byref(info)))
        return info.as_dict()

    def adaptive_info(self, device=-1):
        """kz_adaptive_info: the summary of the replica's last adaptive call, as a dict."""
        info = abi.KzAdaptiveInfo()
        abi.check(self.lib, self.lib.kz_adaptive_info(self.h, int(device), C.byref(info)))
        return info.as_dict()

    def adaptive_stage_ms(self, device=-1):
        """kz_adaptive_stage_ms: device milliseconds of the last adaptive call's (moment resolve, classification, read-back), summed over its rounds."""
        out = (C.c_float * 3)()
        abi.check(self.lib, self.lib.kz_adaptive_stage_ms(self.h, int(device), out))
        return [float(x) for x in out]

    def adaptive_blocks(self, device=-1):
        """kz_adaptive_blocks: the block records of the replica's last adaptive call, 1-D of abi.ADAPTIVE_BLOCK_DTYPE, the frame's blocks row-major."""
        out = np.zeros(self.adaptive_info(device)["blocks"], abi.ADAPTIVE_BLOCK_DTYPE)
        abi.check(self.lib, self.lib.kz_adaptive_blocks(self.h, int(device), out.ctypes.data_as(C.POINTER(abi.KzAdaptiveBlock)), out.size))
        return out

    def adaptive_counts(self, device=-1):
        """kz_adaptive_counts: (h, w) uint32, the samples every frame pixel received in the replica's last adaptive call."""
        out = np.zeros((self.height, self.width), np.uint32)
        abi.check(self.lib, self.lib.kz_adaptive_counts(self.h, int(device), out.ctypes.data_as(abi.u32p), out.size))
        return out

    # ---- the denoiser's history across camera edits (include/kazen_mi355x_temporal.h)
    def _denoise_history(self, entry, device, opts, vargs, targs, rargs=None):
        """denoise_temporal, denoise_motion and (rargs: responsive_opts' arguments) denoise_responsive: the option structs and the call of `entry`."""
        structs = [denoise_opts(**opts), variance_opts(*vargs), temporal_opts(*targs)] + ([] if rargs is None else [responsive_opts(*rargs)])
        abi.check(self.lib, getattr(self.lib, entry)(self.h, -1 if device is None else int(device), *[C.byref(x) for x in structs]))

    def denoise_temporal(self, device=None, sigma_variance=0.0, samples=0, vflags=0, vreserved=0, depth_tolerance=0.0, normal_tolerance=0.0, max_history=0, tflags=0,
                         treserved=(0, 0, 0, 0), **opts):
        """kz_denoise_temporal: denoise_variance() with the replica's history reprojected from the previous call's camera and blended in first; the result is read
        like denoise()'s. Options: denoise_opts', variance_opts' and temporal_opts'."""
        self._denoise_history("kz_denoise_temporal", device, opts, (sigma_variance, samples, vflags, vreserved), (depth_tolerance, normal_tolerance, max_history, tflags, treserved))

    def temporal_info(self, device=-1):
        """kz_temporal_info: (bytes the history holds on that replica, calls folded into it since it last started)."""
        b, n = C.c_uint64(), C.c_uint32()
        abi.check(self.lib, self.lib.kz_temporal_info(self.h, int(device), C.byref(b), C.byref(n)))
        return int(b.value), int(n.value)

    def temporal_reset(self, device=-1):
        abi.check(self.lib, self.lib.kz_temporal_reset(self.h, int(device)))

    def temporal_history(self, device=None):
        """kz_temporal_download: (h, w, 12) = per pixel (e.rgb, v), (n.xyz, z), (N, 0, 0, 0) - what denoise_temporal_films takes as `history`."""
        out = np.zeros((self.height, self.width, 12), np.float32)
        abi.check(self.lib, self.lib.kz_temporal_download(self.h, -1 if device is None else int(device), out.ctypes.data_as(abi.f32p), out.size))
        return out

    # ---- the history kept across set_transforms (include/kazen_mi355x_motion.h)
    def motion_ids(self, device=None):
        """kz_motion_ids: (h, w) uint32, the mesh the centre of every frame pixel shows (abi.KZ_MOTION_MISS: none) - for path_mis behind an invisible light."""
        out = np.zeros((self.height, self.width), np.uint32)
        abi.check(self.lib, self.lib.kz_motion_ids(self.h, -1 if device is None else int(device), out.ctypes.data_as(abi.u32p), out.size))
        return out

    def denoise_motion(self, device=None, sigma_variance=0.0, samples=0, vflags=0, vreserved=0, depth_tolerance=0.0, normal_tolerance=0.0, max_history=0, tflags=0,
                       treserved=(0, 0, 0, 0), **opts):
        """kz_denoise_motion: denoise_temporal() whose history survives set_transforms - every pixel looks its history up where its mesh was. Options and results as
        denoise_temporal's; temporal_info / temporal_reset / temporal_history serve both."""
        self._denoise_history("kz_denoise_motion", device, opts, (sigma_variance, samples, vflags, vreserved), (depth_tolerance, normal_tolerance, max_history, tflags, treserved))

    def motion_info(self, device=-1):
        """kz_motion_info: (bytes the id plane and the row table hold on that replica, (static, moved, untracked) meshes of its last denoise_motion)."""
        b, n = C.c_uint64(), (C.c_uint32 * 3)()
        abi.check(self.lib, self.lib.kz_motion_info(self.h, int(device), C.byref(b), n))
        return int(b.value), tuple(int(x) for x in n)

    # ---- a fast history that clamps the long one where the light moved (include/kazen_mi355x_responsive.h)
    def denoise_responsive(self, device=None, sigma_variance=0.0, samples=0, vflags=0, vreserved=0, depth_tolerance=0.0, normal_tolerance=0.0, max_history=0, tflags=0,
                           treserved=(0, 0, 0, 0), fast_history=0, clamp_sigma=0.0, radius=0, clamp=True, rflags=None, rreserved=(0, 0, 0, 0), **opts):
        """kz_denoise_responsive: denoise_motion() with a fast history beside the long one; where the long history's colour leaves the fast one's local mean +- clamp_sigma
        deviations it is clamped and the pixel re-converges in fast_history calls. Options: denoise_motion's and responsive_opts'; results as denoise_temporal's."""
        self._denoise_history("kz_denoise_responsive", device, opts, (sigma_variance, samples, vflags, vreserved), (depth_tolerance, normal_tolerance, max_history, tflags, treserved),
                              (fast_history, clamp_sigma, radius, clamp, rflags, rreserved))

    def responsive_fast(self, device=None):
        """kz_responsive_download: (h, w, 4) = per pixel (f.rgb, vf), the fast history that goes with temporal_history() - what denoise_responsive_films takes as `fast`."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        abi.check(self.lib, self.lib.kz_responsive_download(self.h, -1 if device is None else int(device), out.ctypes.data_as(abi.f32p), out.size))
        return out

    def responsive_info(self, device=-1):
        """kz_responsive_info: bytes the fast planes hold on that replica."""
        b = C.c_uint64()
        abi.check(self.lib, self.lib.kz_responsive_info(self.h, int(device), C.byref(b)))
        return int(b.value)

    def bsdf_query(self, bsdf, wi, wo, acc, s3, uv=None):
        """eval (n,3), pdf (n,), sample (n,8) = weight rgb, wo xyz, alive, pdf(bRec) after sample()."""
        bsdf = np.ascontiguousarray(bsdf, np.int32)
        n = bsdf.shape[0]
        wi, wo, s3 = (np.ascontiguousarray(a, np.float32) for a in (wi, wo, s3))
        acc = np.ascontiguousarray(acc, np.float32)
        uv = None if uv is None else np.ascontiguousarray(uv, np.float32)
        ev, pd, sm = np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros((n, 8), np.float32)
        f = lambda a: a.ctypes.data_as(abi.f32p)
        abi.check(self.lib, self.lib.kz_bsdf_query(self.h, n, bsdf.ctypes.data_as(C.POINTER(C.c_int32)), f(wi), f(wo), f(acc), f(s3),
                                                   None if uv is None else f(uv), f(ev), f(pd), f(sm)))
        return ev, pd, sm

    def texture_query(self, tex, uv):
        tex = np.ascontiguousarray(tex, np.int32)
        uv = np.ascontiguousarray(uv, np.float32)
        out = np.zeros((tex.shape[0], 3), np.float32)
        abi.check(self.lib, self.lib.kz_texture_query(self.h, tex.shape[0], tex.ctypes.data_as(C.POINTER(C.c_int32)), uv.ctypes.data_as(abi.f32p),
                                                      out.ctypes.data_as(abi.f32p)))
        return out

    def camera_rays(self, sxy, axy=None):
        """Camera::sampleRay for pixel-sample positions sxy (n,2) and aperture samples axy (n,2) -> (n,8) = o, d, mint, maxt."""
        sxy = np.ascontiguousarray(sxy, np.float32)
        axy = None if axy is None else np.ascontiguousarray(axy, np.float32)
        out = np.zeros((sxy.shape[0], 8), np.float32)
        f = lambda a: a.ctypes.data_as(abi.f32p)
        abi.check(self.lib, self.lib.kz_camera_rays(self.h, sxy.shape[0], f(sxy), None if axy is None else f(axy), f(out)))
        return out

    def light_query(self, light, ref, u3):
        """AreaLight::sample of light rows from ref with Mesh::sample's three draws -> (n,14) = p, n, wi, pdf, eval/pdf, triangle."""
        light = np.ascontiguousarray(light, np.int32)
        ref, u3 = np.ascontiguousarray(ref, np.float32), np.ascontiguousarray(u3, np.float32)
        out = np.zeros((light.shape[0], 14), np.float32)
        f = lambda a: a.ctypes.data_as(abi.f32p)
        abi.check(self.lib, self.lib.kz_light_query(self.h, light.shape[0], light.ctypes.data_as(C.POINTER(C.c_int32)), f(ref), f(u3), f(out)))
        return out

    def srgb8(self):
        """(h, w, 3) uint8: the raster Bitmap::savePNG writes (bitmap.cpp:39-62), resolved on the device."""
        out = np.zeros((self.height, self.width, 3), np.uint8)
        abi.check(self.lib, self.lib.kz_film_to_srgb8(self.h, out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size))
        return out

    def set_stats(self, enable=True):
        abi.check(self.lib, self.lib.kz_set_stats(self.h, 1 if enable else 0))

    def stats(self, reset=False):
        s = abi.KzStats()
        abi.check(self.lib, self.lib.kz_get_stats(self.h, C.byref(s), 1 if reset else 0))
        return s.as_dict()

    def last_stage_ms(self):
        out = np.zeros(6, np.float32)
        abi.check(self.lib, self.lib.kz_last_stage_ms(self.h, out.ctypes.data_as(abi.f32p)))
        d = dict(zip(("generate", "trace_bounce", "shade", "trace_shadow", "film", "trace_camera"), [round(float(x), 3) for x in out]))
        d["trace_closest"] = round(d["trace_bounce"] + d["trace_camera"], 3)
        return d

    def last_kernel_ms(self):
        ms = C.c_float()
        abi.check(self.lib, self.lib.kz_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value


def denoise_opts(iterations=0, guides=0, demodulate=True, use_guides=True, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0, flags=None, reserved=0):
    """A KzDenoiseOpts: 0 means the default (5 iterations; every available guide; sigmas 1.0, 0.3, 0.1, 0.1). guides: names or the KZ_AOV_* mask;
    demodulate=False / use_guides=False set KZ_DENOISE_NO_DEMODULATE / KZ_DENOISE_NO_GUIDES (`flags` overrides the two)."""
    if flags is None:
        flags = (0 if demodulate else abi.KZ_DENOISE_NO_DEMODULATE) | (0 if use_guides else abi.KZ_DENOISE_NO_GUIDES)
    return abi.KzDenoiseOpts(int(iterations), Scene._aov_mask(guides), int(flags), int(reserved), float(sigma_color), float(sigma_normal), float(sigma_depth), float(sigma_albedo))


def denoise_films(film, albedo=None, normal=None, depth=None, border=0, device=0, lib=None, **opts):
    """kz_denoise_films: the device's denoiser on host films of (h + 2 border, w + 2 border, 4) float32 each (albedo / normal / depth may be None: an absent
    guide); needs a device, no scene. Returns the denoised film, same shape."""
    lib = lib or abi.load_library()
    film, g, frame = _host_films(film, (albedo, normal, depth), border, "a guide film has the picture's shape")
    out = np.empty_like(film)
    o = denoise_opts(**opts)
    abi.check(lib, lib.kz_denoise_films(int(device), *frame, film.ctypes.data_as(abi.f32p), *[None if a is None else a.ctypes.data_as(abi.f32p) for a in g],
                                        C.byref(o), out.ctypes.data_as(abi.f32p)))
    return out


def _host_films(film, others, border, shape_error):
    """The picture and the films that go with it (None: absent) as contiguous float32 arrays of one shape, and the frame (width, height, border) they hold."""
    film = np.ascontiguousarray(film, np.float32)
    if film.ndim != 3 or film.shape[2] != 4:
        raise ValueError("a film is (h + 2 border, w + 2 border, 4)")
    g = [None if a is None else np.ascontiguousarray(a, np.float32) for a in others]
    for a in g:
        if a is not None and a.shape != film.shape:
            raise ValueError(shape_error)
    return film, g, (film.shape[1] - 2 * int(border), film.shape[0] - 2 * int(border), int(border))


def variance_opts(sigma_variance=0.0, samples=0, flags=0, reserved=0):
    """A KzVarianceOpts: 0 means the default (sigma 3.0; the replica's sample count)."""
    return abi.KzVarianceOpts(float(sigma_variance), int(samples), int(flags), int(reserved))


def denoise_variance_films(film, moment, albedo=None, normal=None, depth=None, border=0, device=0, lib=None, sigma_variance=0.0, samples=0, vflags=0, vreserved=0,
                           return_variance=False, **opts):
    """kz_denoise_variance_films: the device's variance-guided denoiser on host films (denoise_films' layout; `moment`: the second-moment film; `samples` must be
    stated). Returns the denoised film, or (film, v_last of shape (h, w)) with return_variance."""
    lib = lib or abi.load_library()
    film, g, frame = _host_films(film, (moment, albedo, normal, depth), border, "the moment film and the guide films have the picture's shape")
    out = np.empty_like(film)
    var = np.full((max(frame[1], 0), max(frame[0], 0)), np.nan, np.float32) if return_variance else None
    o, v = denoise_opts(**opts), variance_opts(sigma_variance, samples, vflags, vreserved)
    abi.check(lib, lib.kz_denoise_variance_films(int(device), *frame, film.ctypes.data_as(abi.f32p), *[None if a is None else a.ctypes.data_as(abi.f32p) for a in g],
                                                 C.byref(o), C.byref(v), out.ctypes.data_as(abi.f32p), None if var is None else var.ctypes.data_as(abi.f32p)))
    return (out, var) if return_variance else out


def adaptive_opts(threshold, floor=0.0, min_samples=0, max_samples=0, step=0, block=0, outlier_permille=0, flags=0):
    """A KzAdaptiveOpts (include_ext/kazen_mi355x_adaptive.h): threshold has no default; 0 elsewhere means the default (floor 0.01, min(16, max) samples before the
    first test, the scene's sample count as the cap, doubling rounds, blocks of 16 pixels, no outliers)."""
    return abi.KzAdaptiveOpts(float(threshold), float(floor), int(min_samples), int(max_samples), int(step), int(block), int(outlier_permille), int(flags))


def adaptive_schedule(scene_samples, threshold=1.0, lib=None, **opts):
    """kz_adaptive_schedule: the round ends n_0 < n_1 < ... = the cap of a call that converges nowhere, as a list."""
    lib = lib or abi.load_library()
    a, n = adaptive_opts(threshold, **opts), C.c_uint32()
    abi.check(lib, lib.kz_adaptive_schedule(C.byref(a), int(scene_samples), None, 0, C.byref(n)))
    out = (C.c_uint32 * max(1, n.value))()
    abi.check(lib, lib.kz_adaptive_schedule(C.byref(a), int(scene_samples), out, n.value, C.byref(n)))
    return [int(out[i]) for i in range(n.value)]


def adaptive_tiles(width, height, block, active, lib=None):
    """kz_adaptive_tiles: the tile list [(x0, y0, w, h)] of the blocks whose entry of `active` (block rows x block columns, row-major) is non-zero."""
    lib = lib or abi.load_library()
    act = np.ascontiguousarray(np.asarray(active).ravel() != 0, np.uint8)
    if act.size != ((int(width) + int(block) - 1) // int(block)) * ((int(height) + int(block) - 1) // int(block)):
        raise ValueError("active: one entry per block of the frame")
    ptr, n = act.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_uint32()
    abi.check(lib, lib.kz_adaptive_tiles(int(width), int(height), int(block), ptr, None, 0, C.byref(n)))
    out = (abi.KzTile * max(1, n.value))()
    abi.check(lib, lib.kz_adaptive_tiles(int(width), int(height), int(block), ptr, out, n.value, C.byref(n)))
    return [(t.x0, t.y0, t.w, t.h) for t in out[:n.value]]


def adaptive_classify_films(film, moment, block_samples, threshold, border=0, device=0, lib=None, **opts):
    """kz_adaptive_classify_films, the test surface: the device's classification stage on host films (denoise_films' layout) with `block_samples` (one n per block,
    row-major; 0 = skipped). Returns the records, 1-D of abi.ADAPTIVE_BLOCK_DTYPE. max_samples = 0 here: no cap is known."""
    lib = lib or abi.load_library()
    film, (moment,), frame = _host_films(film, (moment,), border, "the moment film has the picture's shape")
    a = adaptive_opts(threshold, **opts)
    e = a.block or 16
    ns = np.ascontiguousarray(np.asarray(block_samples).ravel(), np.uint32)
    if e in (8, 16, 32, 64) and ns.size != ((frame[0] + e - 1) // e) * ((frame[1] + e - 1) // e):      # (another edge: the library refuses it by name)
        raise ValueError("block_samples: one entry per block of the frame")
    out = np.zeros(ns.size, abi.ADAPTIVE_BLOCK_DTYPE)
    abi.check(lib, lib.kz_adaptive_classify_films(int(device), *frame, film.ctypes.data_as(abi.f32p), moment.ctypes.data_as(abi.f32p), ns.ctypes.data_as(abi.u32p), C.byref(a),
                                                  out.ctypes.data_as(C.POINTER(abi.KzAdaptiveBlock))))
    return out


def temporal_opts(depth_tolerance=0.0, normal_tolerance=0.0, max_history=0, flags=0, reserved=(0, 0, 0, 0)):
    """A KzTemporalOpts: 0 means the default (depth tolerance 0.05 relative, normal tolerance 0.5, a history of 32 calls)."""
    return abi.KzTemporalOpts(float(depth_tolerance), float(normal_tolerance), int(max_history), int(flags), (C.c_uint32 * 4)(*[int(r) for r in reserved]))


def temporal_view(camera, lib=None):
    """kz_temporal_view: the KzTemporalView of a camera given as SceneDescription.camera gives it (a dict). Needs no device."""
    from .scenes import camera_to_c
    lib = lib or abi.load_library()
    cam = dict(camera)
    if "toWorld" in cam:
        cam["toWorld"] = np.array(cam["toWorld"], np.float32)
    c = camera_to_c(cam, abi.KzCamera())
    view = abi.KzTemporalView()
    abi.check(lib, lib.kz_temporal_view(C.byref(c), C.byref(view)))
    view._camera = c                                                    # (keeps what the C camera points to alive with the view)
    return view


def _history_films(entry, film, moment, albedo, normal, depth, border, device, lib, vargs, targs, current, previous, history, return_variance, opts, motion=None,
                   responsive=None):
    """What denoise_temporal_films, denoise_motion_films (motion = (ids, rows, n_rows)) and denoise_responsive_films (responsive = (fast, responsive_opts' arguments)
    as well) share: the shape checks, the output buffers, the option structs and the call of `entry`. Returns (film, history[, fast][, v_last])."""
    lib = lib or abi.load_library()
    film, g, frame = _host_films(film, (moment, albedo, normal, depth), border, "the moment film and the guide films have the picture's shape")
    h, w = max(frame[1], 0), max(frame[0], 0)
    if history is not None:
        history = np.ascontiguousarray(history, np.float32)
        if history.shape != (h, w, 12):
            raise ValueError("a history is (h, w, 12)")
    fast = responsive[0] if responsive else None
    if fast is not None:
        fast = np.ascontiguousarray(fast, np.float32)
        if fast.shape != (h, w, 4):
            raise ValueError("a fast plane is (h, w, 4)")
    if motion:
        ids, rows, n_rows = motion
        if ids is not None:
            ids = np.ascontiguousarray(ids, np.uint32)
            if ids.shape != (h, w):
                raise ValueError("ids are (h, w)")
        if n_rows is None:
            n_rows = 0 if rows is None else getattr(rows, "n_rows", len(rows))
    out = np.empty_like(film)
    hist = np.full((h, w, 12), np.nan, np.float32)
    fout = np.full((h, w, 4), np.nan, np.float32) if responsive else None
    var = np.full((h, w), np.nan, np.float32) if return_variance else None
    o, v, t = denoise_opts(**opts), variance_opts(*vargs), temporal_opts(*targs)
    p = lambda a: None if a is None else a.ctypes.data_as(abi.f32p)
    args = [int(device), *frame, p(film), *[p(a) for a in g], C.byref(o), C.byref(v), C.byref(t), None if current is None else C.byref(current),
            None if previous is None else C.byref(previous), p(history)]
    if motion:
        args += [None if ids is None else ids.ctypes.data_as(abi.u32p), rows, int(n_rows)]
    args += [p(out), p(hist), p(var)]
    if responsive:
        r = responsive_opts(*responsive[1])
        args += [C.byref(r), p(fast), p(fout)]
    abi.check(lib, getattr(lib, entry)(*args))
    return tuple(a for a in (out, hist, fout, var) if a is not None)


def denoise_temporal_films(film, moment, albedo=None, normal=None, depth=None, border=0, device=0, lib=None, sigma_variance=0.0, samples=0, vflags=0, vreserved=0,
                           depth_tolerance=0.0, normal_tolerance=0.0, max_history=0, tflags=0, treserved=(0, 0, 0, 0), current=None, previous=None, history=None,
                           return_variance=False, **opts):
    """kz_denoise_temporal_films: the device's temporal stage and variance-guided denoiser on host films (denoise_variance_films' layout; `depth` and `samples` must be
    given). current / previous: KzTemporalView of this frame and of `history` ((h, w, 12) as Scene.temporal_history gives it; None: no history).
    Returns (film, history (h, w, 12)), or (film, history, v_last (h, w)) with return_variance."""
    return _history_films("kz_denoise_temporal_films", film, moment, albedo, normal, depth, border, device, lib, (sigma_variance, samples, vflags, vreserved),
                          (depth_tolerance, normal_tolerance, max_history, tflags, treserved), current, previous, history, return_variance, opts)


def motion_rows(cur, prev, lib=None):
    """kz_motion_rows: the KzMotionRow table (a ctypes array) of meshes whose object-to-world matrices are `cur` now and were `prev` when the history was stored:
    (n, 4, 4) arrays, or None for identities (then the other one gives n). Needs no device."""
    lib = lib or abi.load_library()
    mats = [None if m is None else np.ascontiguousarray(m, np.float32).reshape(-1, 16) for m in (cur, prev)]
    n = max([m.shape[0] for m in mats if m is not None] or [0])
    if any(m is not None and m.shape[0] != n for m in mats):
        raise ValueError("cur and prev hold one matrix per mesh")
    rows = (abi.KzMotionRow * max(1, n))()
    abi.check(lib, lib.kz_motion_rows(*[None if m is None else m.ctypes.data_as(abi.f32p) for m in mats], n, rows))
    rows.n_rows = n
    return rows


def denoise_motion_films(film, moment, albedo=None, normal=None, depth=None, border=0, device=0, lib=None, sigma_variance=0.0, samples=0, vflags=0, vreserved=0,
                         depth_tolerance=0.0, normal_tolerance=0.0, max_history=0, tflags=0, treserved=(0, 0, 0, 0), current=None, previous=None, history=None,
                         ids=None, rows=None, n_rows=None, return_variance=False, **opts):
    """kz_denoise_motion_films: denoise_temporal_films with the motion stage - ids (h, w) uint32 (abi.KZ_MOTION_MISS: a miss) and rows, a KzMotionRow array as
    motion_rows gives it (n_rows: its length, when it is not motion_rows'). Returns what denoise_temporal_films returns."""
    return _history_films("kz_denoise_motion_films", film, moment, albedo, normal, depth, border, device, lib, (sigma_variance, samples, vflags, vreserved),
                          (depth_tolerance, normal_tolerance, max_history, tflags, treserved), current, previous, history, return_variance, opts, motion=(ids, rows, n_rows))


def responsive_opts(fast_history=0, clamp_sigma=0.0, radius=0, clamp=True, flags=None, reserved=(0, 0, 0, 0)):
    """A KzResponsiveOpts: 0 means the default (a fast history of 2 calls, mean +- 2.0 deviations, radius 1: a 3 x 3 window; DESIGN.md 4i has the sweep). clamp=False sets
    KZ_RESPONSIVE_CLAMP_OFF (`flags` overrides it)."""
    if flags is None:
        flags = 0 if clamp else abi.KZ_RESPONSIVE_CLAMP_OFF
    return abi.KzResponsiveOpts(int(fast_history), float(clamp_sigma), int(radius), int(flags), (C.c_uint32 * 4)(*[int(r) for r in reserved]))


def denoise_responsive_films(film, moment, albedo=None, normal=None, depth=None, border=0, device=0, lib=None, sigma_variance=0.0, samples=0, vflags=0, vreserved=0,
                             depth_tolerance=0.0, normal_tolerance=0.0, max_history=0, tflags=0, treserved=(0, 0, 0, 0), current=None, previous=None, history=None,
                             ids=None, rows=None, n_rows=None, fast=None, fast_history=0, clamp_sigma=0.0, radius=0, clamp=True, rflags=None, rreserved=(0, 0, 0, 0),
                             return_variance=False, **opts):
    """kz_denoise_responsive_films: denoise_motion_films with the fast history - `fast` (h, w, 4) as Scene.responsive_fast gives it (None: absent) and responsive_opts'
    options. Returns (film, history (h, w, 12), fast (h, w, 4)), or (film, history, fast, v_last (h, w)) with return_variance."""
    return _history_films("kz_denoise_responsive_films", film, moment, albedo, normal, depth, border, device, lib, (sigma_variance, samples, vflags, vreserved),
                          (depth_tolerance, normal_tolerance, max_history, tflags, treserved), current, previous, history, return_variance, opts, motion=(ids, rows, n_rows),
                          responsive=(fast, (fast_history, clamp_sigma, radius, clamp, rflags, rreserved)))


def hits_to_arrays(hits, n):
    raw = np.frombuffer(hits, dtype=np.uint8).reshape(n, C.sizeof(abi.KzHit))
    w = C.sizeof(abi.KzHit) // 4
    f = raw.view(np.float32).reshape(n, w)
    i = raw.view(np.int32).reshape(n, w)
    return {"t": f[:, 0].copy(), "u": f[:, 1].copy(), "v": f[:, 2].copy(), "mesh": i[:, 3].copy(), "prim": i[:, 4].copy(),
            "p": f[:, 5:8].copy(), "uv": f[:, 8:10].copy(), "sh_s": f[:, 10:13].copy(), "sh_t": f[:, 13:16].copy(),
            "sh_n": f[:, 16:19].copy(), "geo_n": f[:, 19:22].copy()}
