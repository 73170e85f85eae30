"""Webui-side registrations beyond the SdUnet / SdOptimization / VAE hooks (boundaries B3, B5, B6 of INTEGRATION.md), as functions
the shipped extension script calls with the webui's OWN modules as arguments — so a CPU test can drive them with stubs.

  B3  bind_shared           the engine samplers read ``modules.shared.opts / state / cmd_opts`` (the user's sampler settings, Interrupt /
                            Skip, progress, live preview) instead of the package's standalone defaults.
      install_samplers      every row of ``modules.sd_samplers.all_samplers`` (modules/sd_samplers.py:11-16) whose name the engine's
                            sampler table carries gets a constructor that returns the engine sampler (fused CFG / step kernels) WHILE
                            the engine UNet is the active ``sd_unet.current_unet`` and no cfg_denoiser / cfg_denoised / cfg_after_cfg /
                            extra_noise script callback is registered, and the stock torch sampler otherwise: same names, aliases and
                            options, so scripts / API / infotext are untouched.  ToMe / Hypertile jobs are refused (they patch torch
                            modules the engine UNet replaces); a refiner-checkpoint job is forwarded to the stock sampler.
  B5  install_lora_hook     wraps ``networks.load_networks`` of extensions-builtin/Lora (called from ExtraNetworkLora.activate,
                            extra_networks_lora.py:18-45): the stock function keeps the text-encoder part and the bookkeeping, then the
                            UNet part of the same network files is merged on the GPU into the engine's packed weights.
  B6  install_clip_hook     points ``encode_with_transformers`` of every text-encoder wrapper of the loaded model — CLIP-L of SD 1.x
                            (modules/sd_hijack_clip.py:351-360), OpenCLIP-H of SD 2.x (sd_hijack_open_clip.py:26-30), CLIP-L + OpenCLIP-bigG
                            of SDXL (sd_hijack_clip.py:369-377, sd_hijack_open_clip.py:57-66) — at the engine's tower; tokenisation,
                            chunking, emphasis and textual inversion stay.

``EngineModelView`` is what those see as "the model": the webui's LatentDiffusion object supplies the schedule and the flags, the
active ``Mi355xUnet`` supplies the engine and the checkpoint weights (the LoRA "weights backup").
"""
from __future__ import annotations

import types
from typing import Optional


class EngineModelView:
    """The attribute set stable-diffusion-webui_amd's samplers / networks read from a model (sd_models.SdModel), served from the
    webui's ``shared.sd_model`` + the active engine UNet."""

    def __init__(self, sd_model, unet):
        import torch
        self._sd_model, self._unet = sd_model, unet
        self.engine = unet.engine
        self.device = torch.device("cuda", unet.engine.device)
        self.unet_cfg = unet.unet_cfg
        self.is_sdxl = bool(getattr(sd_model, "is_sdxl", False))
        self.is_sdxl_inpaint = bool(getattr(sd_model, "is_sdxl_inpaint", False))
        self.parameterization = getattr(sd_model, "parameterization", "eps")
        self.cond_stage_key = getattr(sd_model, "cond_stage_key", "txt")
        inner = getattr(sd_model, "model", None)
        self.model = types.SimpleNamespace(conditioning_key=getattr(inner, "conditioning_key", "crossattn"))
        self.scale_factor = getattr(sd_model, "scale_factor", 0.18215)

    @property
    def alphas_cumprod(self):                                 # read per job: the webui rewrites it for the schedule overrides
        return self._sd_model.alphas_cumprod

    @property
    def cond_stage_model_empty_prompt(self):
        return getattr(self._sd_model, "cond_stage_model_empty_prompt", None)

    def unet_checkpoint_tensor(self, engine_key: str):
        from . import schema
        return self._unet.checkpoint()[schema.UNET_PREFIX + engine_key]

    def decode_first_stage(self, z):
        return self._sd_model.decode_first_stage(z)

    def encode_first_stage(self, x):
        return self._sd_model.encode_first_stage(x)

    def get_first_stage_encoding(self, e):
        return self._sd_model.get_first_stage_encoding(e)


def active_engine_unet(sd_unet_module):
    """The engine UNet if it is the one the webui currently routes UNetModel.forward to (modules/sd_unet.py:86-93), else None."""
    from .sd_unet import Mi355xUnet
    cur = getattr(sd_unet_module, "current_unet", None)
    return cur if isinstance(cur, Mi355xUnet) and cur.engine is not None else None


_view_cache = {}


def engine_model_view(sd_model, sd_unet_module) -> Optional[EngineModelView]:
    unet = active_engine_unet(sd_unet_module)
    if unet is None:
        return None
    key = (id(sd_model), id(unet), id(unet.engine))
    view = _view_cache.get(key)
    if view is None:
        _view_cache.clear()
        view = _view_cache[key] = EngineModelView(sd_model, unet)
    return view


# ---- B3 ---------------------------------------------------------------------------------------------------------------------------
def bind_shared(webui_shared, webui_sd_samplers_common=None, webui_scripts=None):
    """The engine samplers read the webui's OWN ``opts`` / ``state`` / ``cmd_opts`` / ``total_tqdm`` from here on (shared.bind_webui),
    store their x0 predictions through the webui's ``store_latent`` (live preview, modules/sd_samplers_common.py:115-120) and hand
    ``Script.on_mask_blend`` the webui's ``MaskBlendArgs`` (modules/scripts.py:16-26)."""
    from . import shared
    shared.bind_webui(webui_shared, getattr(webui_sd_samplers_common, "store_latent", None), getattr(webui_scripts, "MaskBlendArgs", None))


SAMPLER_CALLBACK_LISTS = ("callbacks_cfg_denoiser", "callbacks_cfg_denoised", "callbacks_cfg_after_cfg", "callbacks_extra_noise")


def registered_sampler_callbacks(script_callbacks) -> list:
    """Names of the per-step script callback lists that are not empty (modules/script_callbacks.py:219-230, fired at
    modules/sd_samplers_cfg_denoiser.py:212, 279, 307 and modules/sd_samplers_kdiffusion.py:146-151).  They receive — and may rewrite —
    the torch tensors of the reference's CFG denoiser (x_in, sigma_in, the cond batch, x_out, denoised); the fused CFG kernels have
    no such tensors to offer, so a job that would fire any of them runs the stock sampler."""
    table = getattr(script_callbacks, "callback_map", None) or {}
    return [name for name in SAMPLER_CALLBACK_LISTS if table.get(name)]


def hypertile_active(torch_module) -> bool:
    """extensions-builtin/hypertile/hypertile.py:318-347: ``hypertile_hook_model(module, ...)`` wraps the self-attention forwards below
    ``module`` (``sd_model.model`` for the U-Net, ``sd_model.first_stage_model`` for the VAE) and marks each wrapped layer with
    ``__webui_hypertile_params``; the tiling is live while any of them has ``enabled`` set."""
    layers = getattr(torch_module, "__webui_hypertile_layers", None)
    if not layers:
        return False
    cached = _hypertile_params.get(id(layers))
    if cached is None or cached[0] is not layers:
        cached = _hypertile_params[id(layers)] = (layers, [getattr(m, "__webui_hypertile_params") for n, m in torch_module.named_modules()
                                                           if n in layers and hasattr(m, "__webui_hypertile_params")])
    return any(getattr(prm, "enabled", False) for prm in cached[1])


def hypertile_unet_active(sd_model) -> bool:
    """opts.hypertile_enable_unet, or the second-pass option inside a hires pass (hypertile_script.py:17-42)."""
    return hypertile_active(getattr(sd_model, "model", None))


_hypertile_params = {}


def patched_unet_reason(sd_model):
    """Why the torch UNet of ``sd_model`` currently computes something the engine UNet does not: token merging
    (modules/sd_models.py:1011-1034 ``tomesd.apply_patch``: merges tokens around attn1) or Hypertile (tiled self-attention).  Both patch
    torch modules the engine never calls, so the engine refuses the job instead of silently ignoring them."""
    if getattr(sd_model, "applied_token_merged_ratio", 0) > 0:
        return f"token merging is active (ratio {sd_model.applied_token_merged_ratio})"
    if hypertile_unet_active(sd_model):
        return "Hypertile is enabled for the U-Net"
    return None


REFUSAL = ("{why}: it patches the torch UNet, which the [MI355X] SD Unet replaces, and the webui's torch UNet cannot be reached from here. "
           "Set Settings -> SD Unet to None for this job (the mi355x cross-attention optimization keeps working inside the torch UNet), "
           "or turn the feature off.")

_webui_sd_unet = None


def webui_sd_unet_module():
    """modules.sd_unet of the webui this package is bound to (install_samplers / install_lora_hook were handed it), else an imported one."""
    if _webui_sd_unet is not None:
        return _webui_sd_unet
    import sys
    return sys.modules.get("modules.sd_unet")


def job_needs_torch_unet(p, sd_model):
    """Why this sampling call must run on the webui's torch UNet: ToMe / Hypertile patch it (including the hires-pass ratios that are
    applied after the sampler was built: modules/processing.py:1442).  Such a call goes to the stock sampler, and every UNet evaluation
    under it to the patched torch UNet (Mi355xUnet._torch_unet_forward) — SURVEY.md section 7 (vi): fall back, never ignore."""
    from . import shared
    why = patched_unet_reason(sd_model)
    if why is None and hasattr(p, "get_token_merging_ratio"):
        ratio = p.get_token_merging_ratio(for_hr=bool(getattr(p, "is_hr_pass", False)))
        why = f"token merging is requested (ratio {ratio})" if ratio and ratio > 0 else None
    if why is None and getattr(p, "is_hr_pass", False) and getattr(shared.opts, "hypertile_enable_unet_secondpass", False):
        why = "Hypertile is enabled for the U-Net second pass"
    if why is None and getattr(shared.opts, "hypertile_enable_unet", False):
        why = "Hypertile is enabled for the U-Net"
    return why


def job_needs_stock_sampler(p, sd_model=None):
    """Per-job reasons (only ``p`` knows them, and ``p`` is not there yet when the row's constructor runs) to hand a sampling call to
    the stock sampler: a refiner CHECKPOINT switch while the webui's checkpoint loader is out of reach (install_refiner_switch binds it:
    round 6 — until then such jobs always went to the stock sampler), or a torch UNet that ToMe / Hypertile patched."""
    from . import sd_samplers as amd
    if getattr(p, "refiner_checkpoint_info", None) is not None and getattr(p, "refiner_sd_model", None) is None and amd.webui_refiner_switch is None:
        return "refiner checkpoint switch"
    return job_needs_torch_unet(p, sd_model) if sd_model is not None else None


def install_refiner_switch(webui_sd_models, webui_shared, sd_unet_module, webui_devices=None):
    """The refiner CHECKPOINT switch of a webui job on the engine path (modules/sd_samplers_common.py:158-202, statement for statement
    after the progress test the caller already made): the webui reloads its model with the refiner checkpoint
    (``sd_models.reload_model_weights(info=...)`` — which ends in ``sd_unet.apply_unet()``, modules/sd_models.py:1000: with "SD Unet:
    Automatic" that activates the engine UNet listed for the refiner checkpoint, modules/sd_unet.py:14-31), recomputes the conds with the new
    text encoder (``p.setup_conds()``), and the engine sampler continues on the newly activated engine: new model view, new wrapped
    denoiser, the new conds in the sampler loop's extra_args (CFGDenoiser.update_inner_model, modules/sd_samplers_cfg_denoiser.py:93-98).
    If the webui did NOT activate an engine UNet for the refiner checkpoint (the user pinned "SD Unet: None" or another option) the job
    cannot continue on this path and says so."""
    from . import sd_samplers as amd, shared

    def switch(cfg_denoiser, completed_ratio):
        p = cfg_denoiser.p
        opts = shared.opts
        refiner_switch_at = getattr(p, "refiner_switch_at", None)
        info = getattr(p, "refiner_checkpoint_info", None)
        if refiner_switch_at is not None and completed_ratio < refiner_switch_at:
            return False
        if info is None or getattr(webui_shared.sd_model, "sd_checkpoint_info", None) == info:
            return False
        if getattr(p, "enable_hr", False):
            is_second_pass = p.is_hr_pass
            if opts.hires_fix_refiner_pass == "first pass" and is_second_pass:
                return False
            if opts.hires_fix_refiner_pass == "second pass" and not is_second_pass:
                return False
            if opts.hires_fix_refiner_pass != "second pass":
                p.extra_generation_params['Hires refiner'] = opts.hires_fix_refiner_pass
        p.extra_generation_params['Refiner'] = info.short_title
        p.extra_generation_params['Refiner switch at'] = refiner_switch_at
        skip = getattr(webui_sd_models, "SkipWritingToConfig", None)
        if skip is not None:
            with skip():
                webui_sd_models.reload_model_weights(info=info)
        else:
            webui_sd_models.reload_model_weights(info=info)
        if webui_devices is not None and hasattr(webui_devices, "torch_gc"):
            webui_devices.torch_gc()
        p.setup_conds()
        view = engine_model_view(webui_shared.sd_model, sd_unet_module)
        if view is None:
            raise RuntimeError("refiner switch: the webui did not activate an engine UNet for the refiner checkpoint "
                               f"'{info.short_title}' (set 'SD Unet' to Automatic, or to None for this job)")
        sampler = cfg_denoiser.sampler
        sampler.sd_model = view
        shared.sd_model = view
        cfg_denoiser.model_wrap = None                        # rebuilt over the new checkpoint's alphas_cumprod
        cfg_denoiser._ctx_key = None                          # the cached K / V projections belong to the other engine
        cfg_denoiser._cond_sel = cfg_denoiser._uncond_sel = None
        c, uc = p.get_conds()
        args = sampler.sampler_extra_args
        args['cond'], args['uncond'] = c, uc
        args.pop('y', None)
        args.pop('uy', None)                                  # SDXL: the vector conditioning rides inside the dict conds (CFGDenoiser._reconstruct_conds)
        return True
    amd.webui_refiner_switch = switch
    return switch


def uninstall_refiner_switch():
    from . import sd_samplers as amd
    amd.webui_refiner_switch = None


# ---- one webui process, N devices, at the sampler boundary (VERDICT r5 missing #2) -------------------------------
# The webui's own process_images loop stays what it is — one process behind queue_lock (modules/call_queue.py:8-13), one device selected
# (modules/cmd_args.py:106) — so inside a webui the place where a batch can fan out is the sampler row (B3): with opts.mi355x_devices =
# "0,1,.." a row's sample / sample_img2img cuts the batch's ROWS into contiguous ranges, one per device, and runs each range's whole
# sampling loop in a worker thread on that device's own engine UNet (a replica packed from the active Mi355xUnet's checkpoint, LoRA
# merges re-applied).  Images are independent units — own generator (modules/rng.py:108), own cond row, per-image CFG combine — so a
# range's latents are what the single-device call computes for those rows (bit for bit at equal per-call batch size; to fp16 rounding
# otherwise: the tile table follows the GEMM's M).  The decode (B4) stays on the webui's device: 6 % of a job.
_unet_replicas = {}                                           # (id(primary unet), id(its engine), device) -> Mi355xUnet
serial_device_workers = False                                 # tests on the host-emulated tier: workers one after the other


def _torch_device(index: int):
    import torch
    return torch.device("cuda", int(index))


def _unet_on_device(unet, device: int, nth: int = 0):
    """The active engine UNet itself for the FIRST worker on its own device, else a replica of it on ``device`` (packed once per
    checkpoint activation).  ``nth``: which worker of that device asks — an engine serves one caller at a time, so a device named twice
    in opts.mi355x_devices gets a second engine, never two threads on one."""
    from .sd_unet import Mi355xUnet
    if int(device) == int(unet.engine.device) and nth == 0:
        return unet
    key = (id(unet), id(unet.engine), int(device), int(nth))
    rep = _unet_replicas.get(key)
    if rep is None:
        for k in [k for k in _unet_replicas if k[0] == id(unet) and k[1] != id(unet.engine)]:      # replicas of a deactivated engine
            _unet_replicas.pop(k).deactivate()
        rep = Mi355xUnet(unet.checkpoint, unet_cfg=unet.unet_cfg, device_index=int(device))
        rep.activate()
        _unet_replicas[key] = rep
    return rep


def _rows(v, lo, hi, n, device=None):
    """Rows [lo, hi) of one per-image argument of a sampling call: tensors with n leading rows, SDXL dict conds, the webui's
    MulticondLearnedConditioning (.batch list), per-image lists (uncond schedules); anything else is passed as it is."""
    import torch
    if v is None:
        return None
    if torch.is_tensor(v):
        v = v[lo:hi] if v.dim() >= 1 and v.shape[0] == n else v
        return v.to(device) if device is not None else v
    if isinstance(v, dict):
        return {k: _rows(x, lo, hi, n, device) for k, x in v.items()}
    if hasattr(v, "batch") and hasattr(v, "shape") and isinstance(v.batch, list) and len(v.batch) == n:
        return type(v)((hi - lo,) + tuple(v.shape[1:]), v.batch[lo:hi])
    if isinstance(v, (list, tuple)) and len(v) == n:
        return list(v[lo:hi])
    return v


def _job_rows(p, lo, hi, n, device):
    """``p`` as the worker of rows [lo, hi) sees it: batch size, seeds, the per-image tensors of an img2img job, and an ImageRNG over
    ITS seeds in the state the batch's generator is in (the webui drew the initial noise before calling the sampler)."""
    import copy
    from . import rng as amd_rng, shared
    q = copy.copy(p)
    q.batch_size = hi - lo
    for f in ("seeds", "subseeds", "prompts", "negative_prompts"):
        v = getattr(p, f, None)
        if isinstance(v, (list, tuple)) and len(v) == n:
            setattr(q, f, list(v[lo:hi]))
    for f in ("init_latent", "mask", "nmask", "image_conditioning"):
        v = getattr(p, f, None)
        if v is not None:
            setattr(q, f, _rows(v, lo, hi, n, device))
    r = getattr(p, "rng", None)
    if r is not None and hasattr(r, "seeds") and len(r.seeds) == n:
        sub = amd_rng.ImageRNG(r.shape, list(r.seeds[lo:hi]), None if r.subseeds is None else list(r.subseeds[lo:hi]), r.subseed_strength,
                               r.seed_resize_from_h, r.seed_resize_from_w,
                               eta_noise_seed_delta=int(getattr(shared.opts, "eta_noise_seed_delta", 0) or 0), device=device)
        if not getattr(r, "is_first", False):
            sub.next()                                        # the initial noise of these rows: drawn by the webui already
        q.rng = sub
    return q


def sample_over_devices(make_sampler, view, name, p, args, kwargs, devices):
    """One ``sample`` / ``sample_img2img`` call of an engine sampler row with the batch's rows spread over ``devices``."""
    import threading
    import torch
    from . import parallel, shared
    x = args[0]
    n = int(x.shape[0])
    devs = [int(d) for d in devices][:n]
    results, errors = [None] * len(devs), [None] * len(devs)
    lora = getattr(view, "_networks_applied", None)
    # replicas are packed, and the primary engine's LoRA / LyCORIS merges re-applied on them, HERE — one after the other in the calling
    # thread (the network loader keeps module-level state: networks.loaded_networks) — before any worker starts
    views, touched = [], False
    for slot in range(len(devs)):
        dev = _torch_device(devs[slot])
        if torch.cuda.is_available() and dev.type == "cuda":
            torch.cuda.set_device(dev)
        unet = _unet_on_device(view._unet, devs[slot], devs[:slot].count(devs[slot]))
        v = view if unet is view._unet else EngineModelView(view._sd_model, unet)
        if v is not view and lora is not None and getattr(unet, "_networks_applied", None) != lora[0]:
            lora[1](v)
            unet._networks_applied = lora[0]
            touched = True
        views.append(v)
    if touched:
        lora[1](view)                                         # (leaves the loader's module state describing the primary again)
    if torch.cuda.is_available() and x.device.type == "cuda":
        torch.cuda.set_device(x.device)

    def work(slot):
        try:
            lo, hi = parallel.shard_range(n, len(devs), slot)
            dev = _torch_device(devs[slot])
            if torch.cuda.is_available() and dev.type == "cuda":
                torch.cuda.set_device(dev)
            v = views[slot]
            sampler = make_sampler(v)
            sampler.config = getattr(view, "_row_config", None) or getattr(sampler, "config", None)
            q = _job_rows(p, lo, hi, n, dev)
            a = [_rows(v_, lo, hi, n, dev) for v_ in args]
            kw = {k: _rows(v_, lo, hi, n, dev) for k, v_ in kwargs.items()}
            out = getattr(sampler, name)(q, *a, **kw)
            if torch.cuda.is_available() and dev.type == "cuda":
                torch.cuda.synchronize(dev)
            results[slot] = out
        except BaseException as ex:
            errors[slot] = ex
    if serial_device_workers or len(devs) == 1:
        for slot in range(len(devs)):
            work(slot)
    else:
        threads = [threading.Thread(target=work, args=(slot,), name=f"sdmi-sampler-device-{devs[slot]}") for slot in range(len(devs))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    for ex in errors:
        if ex is not None:
            raise ex
    if torch.cuda.is_available() and x.device.type == "cuda":
        torch.cuda.set_device(x.device)
    shared.sd_model = view
    return torch.cat([r.to(x.device) for r in results])


def _engine_sampler_with_job_checks(engine_sampler, stock_ctor, model, make_sampler=None, view=None):
    """``sample`` / ``sample_img2img`` of the engine sampler, preceded by the per-job checks; a job that needs the stock sampler (refiner
    checkpoint switch with the loader out of reach; ToMe / Hypertile on the torch UNet) gets one built on the spot (same row, so same
    config) and the call is forwarded; with several devices in opts.mi355x_devices the batch's rows fan out (sample_over_devices)."""
    for name in ("sample", "sample_img2img"):
        fused = getattr(engine_sampler, name)

        def call(p, *args, _fused=fused, _name=name, **kwargs):
            why = job_needs_stock_sampler(p, model)
            if why is None:
                from .processing import job_devices
                devs = job_devices()
                if make_sampler is not None and view is not None and len(devs) > 1 and args and hasattr(args[0], "shape") and args[0].shape[0] > 1 \
                        and getattr(p, "refiner_checkpoint_info", None) is None:
                    view._row_config = getattr(engine_sampler, "config", None)
                    return sample_over_devices(make_sampler, view, _name, p, args, kwargs, devs)
                return _fused(p, *args, **kwargs)
            stock = stock_ctor(model)
            stock.config = engine_sampler.config
            engine_sampler.stock_delegate, engine_sampler.stock_reason = stock, why
            return getattr(stock, _name)(p, *args, **kwargs)
        setattr(engine_sampler, name, call)
    return engine_sampler


def install_samplers(webui_sd_samplers, sd_unet_module, script_callbacks=None) -> list:
    """Idempotent (the webui re-imports extension scripts on "Reload UI").  Returns the names that now dispatch.  A row builds the
    engine sampler when the engine UNet is the active ``sd_unet.current_unet`` AND no per-step script callback is registered;
    the stock sampler otherwise."""
    from . import sd_samplers as amd, shared
    global _webui_sd_unet
    _webui_sd_unet = sd_unet_module
    replaced = []
    rows = list(webui_sd_samplers.all_samplers)
    for i, row in enumerate(rows):
        mine = amd.all_samplers_map.get(row.name)
        if mine is None:
            continue
        stock = getattr(row.constructor, "_mi355x_stock", row.constructor)

        def constructor(model, stock=stock, mine=mine):
            view = engine_model_view(model, sd_unet_module)
            if view is None or registered_sampler_callbacks(script_callbacks):
                return stock(model)
            shared.sd_model = view                            # what the package's schedulers ask for is_sdxl (sd_schedulers.py)
            return _engine_sampler_with_job_checks(mine.constructor(view), stock, model, make_sampler=mine.constructor, view=view)
        constructor._mi355x_stock = stock
        rows[i] = type(row)(row.name, constructor, row.aliases, row.options)
        replaced.append(row.name)
    webui_sd_samplers.all_samplers[:] = rows
    webui_sd_samplers.all_samplers_map.clear()
    webui_sd_samplers.all_samplers_map.update({x.name: x for x in rows})
    if hasattr(webui_sd_samplers, "set_samplers"):
        webui_sd_samplers.set_samplers()                      # rebuilds samplers / samplers_for_img2img / samplers_map from all_samplers
    return replaced


# ---- B5 ---------------------------------------------------------------------------------------------------------------------------
def install_lora_hook(webui_networks, webui_sd_models, webui_shared, sd_unet_module):
    """``webui_networks`` = the built-in Lora extension's ``networks`` module."""
    from . import networks as amd_networks
    stock = getattr(webui_networks.load_networks, "_mi355x_stock", webui_networks.load_networks)

    files = {}                                                # filename -> (mtime, parsed state dict): a job re-activates the same files

    def on_disk(name):
        """The stock resolution rule (extensions-builtin/Lora/networks.py:303): names that collide with an alias are looked up by
        file name only, everything else through the alias table."""
        forbidden = getattr(webui_networks, "forbidden_network_aliases", {})
        table = webui_networks.available_networks if name.lower() in forbidden else webui_networks.available_network_aliases
        return table.get(name, None)

    def read(filename):
        import os
        try:
            mtime = os.path.getmtime(filename)
        except OSError:
            mtime = None
        hit = files.get(filename)
        if hit is None or hit[0] != mtime:
            hit = files[filename] = (mtime, webui_sd_models.read_state_dict(filename))
        return hit[1]

    def load_networks(names, te_multipliers=None, unet_multipliers=None, dyn_dims=None):
        stock(names, te_multipliers, unet_multipliers, dyn_dims)          # text encoder + loaded_networks bookkeeping as before
        view = engine_model_view(webui_shared.sd_model, sd_unet_module)
        if view is None:
            return
        found = [(n, on_disk(n)) for n in names]
        found = [(n, d) for n, d in found if d is not None]   # the stock loader already reported the missing ones
        idx = {n: i for i, n in enumerate(names)}
        pick = lambda xs: None if not xs else [xs[idx[n]] for n, _ in found]
        te, un, dyn = pick(te_multipliers), pick(unet_multipliers), pick(dyn_dims)
        wanted = tuple((n, d.filename, None if te is None else te[i], None if un is None else un[i], None if dyn is None else dyn[i])
                       for i, (n, d) in enumerate(found))
        if getattr(view, "_networks_request", None) == (wanted, getattr(view.engine, "weights_version", 0)) and \
                all(files.get(d.filename, (None,))[0] == _mtime(d.filename) for _, d in found):
            return                                            # same files, same multipliers, weights untouched since: nothing to merge
        for gone in set(files) - {d.filename for _, d in found}:
            del files[gone]
        names_f, sds_f = [n for n, _ in found], [read(d.filename) for _, d in found]
        amd_networks.load_networks(view, names_f, sds_f, te, un, dyn)
        view._networks_request = (wanted, getattr(view.engine, "weights_version", 0))
        # engine UNet replicas on other devices (sample_over_devices) get the same merges before their next call
        view._networks_applied = (wanted, lambda v, a=(names_f, sds_f, te, un, dyn): amd_networks.load_networks(v, *a))
    load_networks._mi355x_stock = stock
    webui_networks.load_networks = load_networks
    return load_networks


# ---- B6 ---------------------------------------------------------------------------------------------------------------------------
def _clip_embedders(sd_model):
    """The webui's hijacked text-encoder wrappers of a loaded model (modules/sd_hijack.py:205-243): ``cond_stage_model`` itself for
    SD 1.x / 2.x, every wrapped entry of ``conditioner.embedders`` for SDXL."""
    csm = getattr(sd_model, "cond_stage_model", None)
    if csm is None:
        return []
    embedders = getattr(csm, "embedders", None)
    if embedders is None:
        return [csm]
    return [e for e in embedders if hasattr(e, "wrapped") and hasattr(e, "encode_with_transformers")]


def _clip_kind(embedder, is_sdxl: bool):
    """-> (kind, torch text module, token-embedding module) of one wrapper, by STRUCTURE (the class names are the reference's:
    sd_hijack_clip.py:318-377, sd_hijack_open_clip.py:10-71):
      "clip_l"       FrozenCLIPEmbedderWithCustomWords           wrapped.transformer.text_model (transformers CLIPTextModel), SD 1.x
      "clip_l_sdxl"  FrozenCLIPEmbedderForSDXLWithCustomWords    the same tower read at wrapped.layer / layer_idx, SDXL embedder 0
      "openclip"     FrozenOpenCLIPEmbedderWithCustomWords       wrapped.model (open_clip text tower), penultimate layer + ln_final, SD 2.x
      "openclip2"    FrozenOpenCLIPEmbedder2WithCustomWords      wrapped.model, penultimate WITHOUT ln_final + pooled projection, SDXL embedder 1"""
    wrapped = getattr(embedder, "wrapped", None)
    text_model = getattr(getattr(wrapped, "transformer", None), "text_model", None)
    if text_model is not None:
        sdxl_form = is_sdxl or "ForSDXL" in type(embedder).__name__
        return ("clip_l_sdxl" if sdxl_form else "clip_l"), text_model, text_model.embeddings.token_embedding
    model = getattr(wrapped, "model", None)
    if model is not None and hasattr(model, "transformer") and hasattr(model, "token_embedding") and hasattr(model, "ln_final"):
        two = "Embedder2" in type(embedder).__name__ or "Embedder2" in type(wrapped).__name__ or getattr(wrapped, "legacy", True) is False
        return ("openclip2" if two else "openclip"), model, model.token_embedding
    return None, None, None


def install_clip_hook(sd_model, device_index: int = 0, lora_networks=None):
    """Every text tower of the loaded checkpoint is packed into an engine and ``encode_with_transformers`` of ITS wrapper is rebound to
    it: CLIP-L of SD 1.x (sd_hijack_clip.py:351-360), OpenCLIP-H of SD 2.x (sd_hijack_open_clip.py:26-30: the wrapped
    ``encode_with_transformer``, penultimate layer), and both SDXL embedders — CLIP-L read at ``wrapped.layer`` / ``layer_idx``
    (sd_hijack_clip.py:369-377) and OpenCLIP-bigG with its pooled projection (sd_hijack_open_clip.py:57-66); the conditioner that
    concatenates them (modules/sd_models_xl.py:12-34) keeps calling the wrappers.  Token embeddings still come from the webui's
    (textual-inversion patched) embedding layer and enter as ``inputs_embeds``.  A text-encoder LoRA on a tower is merged by the Lora
    extension's own ``network_apply_weights`` (run over the tower's modules when the set of networks touching it changes) and the tower is
    packed again from the merged weights; only a Lora extension without that entry point sends such prompts through the torch tower.
    Returns the encoder (one tower) or the list of encoders (SDXL), None when the checkpoint has no tower this engine knows."""
    from . import schema
    from .engine import Engine
    from .sd_hijack_clip import Mi355xClipTextEncoder
    is_sdxl = bool(getattr(sd_model, "is_sdxl", False))
    made = []
    for emb in _clip_embedders(sd_model):
        kind, tower, tok_emb = _clip_kind(emb, is_sdxl)
        if kind is None:
            continue
        if hasattr(emb, "_mi355x_clip"):
            _unhook(emb)
        wrapped = emb.wrapped

        def packed_tower(kind=kind, tower=tower, wrapped=wrapped):
            """The torch tower's CURRENT weights as an engine tower (whatever the Lora extension has merged into them included)."""
            if kind in ("clip_l", "clip_l_sdxl"):
                cfg = schema.sd15_clip()
                sd = {schema.CLIP_PREFIX + k.replace("token_embedding.wrapped.", "token_embedding."): v for k, v in tower.state_dict().items()}
            else:
                width = int(tower.ln_final.weight.shape[0])
                cfg = schema.openclip_bigg() if width == 1280 else schema.openclip_h()
                raw = {"m." + k: v for k, v in tower.state_dict().items()}
                tew = raw.get("m.token_embedding.wrapped.weight")          # EmbeddingsWithFixes keeps the nn.Embedding as .wrapped
                if tew is not None:
                    raw["m.token_embedding.weight"] = tew
                sd = schema.openclip_to_transformers_keys(raw, "m.")
            return Mi355xClipTextEncoder(Engine(device_index), cfg, sd, layer=getattr(wrapped, "layer", "last"),
                                         layer_idx=getattr(wrapped, "layer_idx", None))
        enc = packed_tower()
        emb._mi355x_clip = enc
        emb._mi355x_clip_networks = ()                        # the text-encoder networks merged into the packed weights
        emb._torch_encode_with_transformers = emb.encode_with_transformers

        def encode_with_transformers(tokens, emb=emb, kind=kind, tok_emb=tok_emb, tower=tower, packed_tower=packed_tower):
            # The Lora extension applies text-encoder deltas lazily, inside the patched torch Linear / MultiheadAttention forwards
            # (extensions-builtin/Lora/networks.py:411-480, 578-605) — forwards the packed tower never runs.  network_apply_weights
            # (:411) is that application for ONE module: restore the backup, add every loaded network's delta IN PLACE, idempotent for
            # an unchanged set.  When the set of networks touching this tower changes, it is run over the tower's modules here and the
            # tower is packed again from the merged weights: the reference's own merge arithmetic, the engine's encoder.
            wanted = text_encoder_networks_request(emb, lora_networks)
            if wanted != emb._mi355x_clip_networks:
                import sys
                apply = getattr(lora_networks if lora_networks is not None else sys.modules.get("networks"), "network_apply_weights", None)
                if apply is None:                             # a Lora extension without that entry point: the torch tower, deltas included
                    return emb._torch_encode_with_transformers(tokens) if wanted else _engine_encode(emb._mi355x_clip, kind, tokens, tok_emb)
                for module in tower.modules():
                    if getattr(module, "network_layer_name", None) is not None:
                        apply(module)
                old = emb._mi355x_clip
                emb._mi355x_clip = packed_tower()
                emb._mi355x_clip_networks = wanted
                if getattr(old, "engine", None) is not None:
                    old.engine.close()
            return _engine_encode(emb._mi355x_clip, kind, tokens, tok_emb)
        emb.encode_with_transformers = encode_with_transformers
        made.append(enc)
    if not made:
        return None
    return made[0] if len(made) == 1 else made


def _engine_encode(enc, kind, tokens, tok_emb):
    e = tok_emb(tokens)                                       # EmbeddingsWithFixes: textual-inversion vectors spliced in
    if kind == "clip_l":
        return enc.encode_with_transformers(tokens, inputs_embeds=e)
    if kind == "clip_l_sdxl":
        return enc.encode_with_transformers_sdxl(tokens, inputs_embeds=e)
    if kind == "openclip":
        return enc.encode_with_transformer_openclip(tokens, inputs_embeds=e)
    return enc.encode_with_transformer_openclip2(tokens, inputs_embeds=e)


def text_encoder_networks_request(cond_stage_model, lora_networks=None) -> tuple:
    """(name, te_multiplier, dyn_dim) of every loaded network of the built-in Lora extension that touches ``cond_stage_model`` with a
    non-zero text-encoder multiplier, in load order: what ``network_apply_weights`` merges into that tower's weights (() = none)."""
    import sys
    lora_networks = lora_networks if lora_networks is not None else sys.modules.get("networks")
    loaded = getattr(lora_networks, "loaded_networks", None)
    if not loaded:
        return ()
    mine, out = None, []
    for net in loaded:
        if not getattr(net, "te_multiplier", 0):
            continue
        for module in getattr(net, "modules", {}).values():
            if mine is None:
                mine = {id(m) for m in cond_stage_model.modules()} if hasattr(cond_stage_model, "modules") else set()
            if id(getattr(module, "sd_module", None)) in mine:
                out.append((getattr(net, "name", None), net.te_multiplier, getattr(net, "dyn_dim", None)))
                break
    return tuple(out)


def text_encoder_networks_active(cond_stage_model, lora_networks=None) -> bool:
    """True while ``networks.loaded_networks`` of the built-in Lora extension holds a network with ``te_multiplier != 0`` and at least
    one module whose ``sd_module`` lives under ``cond_stage_model`` (extensions-builtin/Lora/networks.py:122-147 maps ``lora_te_*`` keys
    to the text encoder's Linear layers)."""
    import sys
    lora_networks = lora_networks if lora_networks is not None else sys.modules.get("networks")
    loaded = getattr(lora_networks, "loaded_networks", None)
    if not loaded:
        return False
    mine = None
    for net in loaded:
        if not getattr(net, "te_multiplier", 0):
            continue
        for module in getattr(net, "modules", {}).values():
            if mine is None:
                mine = {id(m) for m in cond_stage_model.modules()} if hasattr(cond_stage_model, "modules") else set()
            if id(getattr(module, "sd_module", None)) in mine:
                return True
    return False


def _mtime(filename):
    import os
    try:
        return os.path.getmtime(filename)
    except OSError:
        return None


def _unhook(emb):
    if hasattr(emb, "_torch_encode_with_transformers"):
        emb.encode_with_transformers = emb._torch_encode_with_transformers
        emb._mi355x_clip.engine.close()
        del emb._torch_encode_with_transformers, emb._mi355x_clip


def uninstall_clip_hook(sd_model):
    for emb in _clip_embedders(sd_model):
        _unhook(emb)


# ---- image-space upscalers ----------------------------------------------------------------------------------------------------------
def install_esrgan_hook(webui_shared, device_index: int = 0):
    """Point the webui's own ESRGAN / Real-ESRGAN scaler objects at the engine.  Every ``UpscalerData`` of ``webui_shared.sd_upscalers``
    whose scaler class is UpscalerESRGAN or UpscalerRealESRGAN (modules/esrgan_model.py, modules/realesrgan_model.py) keeps its name,
    path resolution and the ``Upscaler.upscale`` driver loop; only ``do_upscale(img, selected_info)`` changes: the checkpoint the stock
    code would load (``load_model``'s local path for ESRGAN, ``UpscalerData.local_data_path`` / ``data_path`` for Real-ESRGAN) runs as
    rrdb_conv launches (RRDBNets) or compact_conv launches (the SRVGGNetCompact models "R-ESRGAN General 4xV3", "General WDN 4xV3" and
    "AnimeVideo") on the image whole instead of as a torch module in tiles.  Whatever the engine cannot take stays on the stock
    path: a checkpoint that is neither a 64 / 32 RRDBNet nor a 64-feature PReLU compact network, or that fails to load or pack for any
    reason, and an image too large for the arena.  Returns the names of the hooked entries."""
    from . import upscaler as amd_upscaler
    engine_scaler = amd_upscaler.UpscalerESRGAN(device_index)
    hooked = []
    for data in getattr(webui_shared, "sd_upscalers", []):
        scaler = getattr(data, "scaler", None)
        if scaler is None or type(scaler).__name__ not in ("UpscalerESRGAN", "UpscalerRealESRGAN"):
            continue
        hooked.append(data.name)
        if hasattr(scaler.do_upscale, "_mi355x_stock"):
            continue
        stock = scaler.do_upscale

        def do_upscale(img, selected_model=None, _stock=stock, _scaler=scaler):
            path = selected_model
            info = next((d for d in getattr(_scaler, "scalers", []) if selected_model in (d.data_path, d.name)), None)
            if info is not None:                                  # Real-ESRGAN's rule: the downloaded file when there is one
                path = getattr(info, "local_data_path", None) or info.data_path
            if isinstance(path, str) and path.startswith("http"):
                return _stock(img, selected_model)                # not on disk yet: the stock code downloads (and runs) it
            try:
                engine_scaler.load_model(path)
            except Exception:                                     # not an RRDBNet the engine is built for (ValueError), a file the
                return _stock(img, selected_model)                # weights-only loader refuses, an engine error: what worked before still works
            try:
                return engine_scaler.do_upscale(img, path)
            except amd_upscaler.EsrganInputTooLarge:
                return _stock(img, selected_model)                # the stock path tiles (ESRGAN_tile) what the arena cannot hold whole
        do_upscale._mi355x_stock = stock
        scaler.do_upscale = do_upscale
    return hooked


def install_swinir_hook(webui_shared, device_index: int = 0):
    """Point the webui's SwinIR scaler objects (extensions-builtin/SwinIR/scripts/swinir_model.py) at the engine: install_esrgan_hook for
    the entries of ``webui_shared.sd_upscalers`` whose scaler class is UpscalerSwinIR.  Name, path / download resolution and the
    ``Upscaler.upscale`` driver loop stay; ``do_upscale(img, model_file)`` runs the checkpoint as sdmi_swinir_run on the image whole
    instead of as a torch module in SWIN_tile tiles; a Swin2SR checkpoint (the ``*.v2.pth`` files the extension builds from
    swinir_model_arch_v2.py, the classical / lightweight Swin2SR models) is recognised by its keys and runs as sdmi_swin2sr_run.  The
    same fall-back rules: a URL that is not on disk yet, a checkpoint the loader refuses (another upsampler or window size, ape, head
    dim > 32) or that fails to load or pack, and an image too large for the arena stay on the stock path.  Returns the names of the
    hooked entries."""
    return _install_whole_image_hook(webui_shared, device_index, "UpscalerSwinIR")


def install_scunet_hook(webui_shared, device_index: int = 0):
    """Point the webui's ScuNET scaler objects (extensions-builtin/ScuNET/scripts/scunet_model.py: "ScuNET GAN", "ScuNET PSNR") at the
    engine: install_swinir_hook for the entries of ``webui_shared.sd_upscalers`` whose scaler class is UpscalerScuNET.
    ``do_upscale(img, selected_file)`` runs the checkpoint as sdmi_scunet_run on the image whole instead of as a torch module in
    SCUNET_tile tiles; the result has the input's size, as the stock model's, and ``Upscaler.upscale`` fits it.  The same fall-back rules:
    a URL that is not on disk yet, a checkpoint the loader refuses (dim other than 64, another window size, a grey-scale model) or that
    fails to load or pack, and an image too large for the arena stay on the stock path.  Idempotent.  Returns the names of the hooked
    entries."""
    return _install_whole_image_hook(webui_shared, device_index, "UpscalerScuNET")


def install_dat_hook(webui_shared, device_index: int = 0):
    """Point the webui's DAT scaler objects (modules/dat_model.py: "DAT x2", "DAT x3", "DAT x4") at the engine: install_swinir_hook for
    the entries of ``webui_shared.sd_upscalers`` whose scaler class is UpscalerDAT.  ``do_upscale(img, path)`` runs the checkpoint as
    sdmi_dat_run on the image whole instead of as a torch module in DAT_tile tiles.  The same fall-back rules: a URL that is not on disk
    yet, a checkpoint the loader refuses (pixelshuffledirect, 3conv, head dim > 32, an odd head count, another split, num_feat other
    than 64) or that fails to load or pack, and an image too large for the arena stay on the stock path.  Idempotent.  Returns the names
    of the hooked entries."""
    return _install_whole_image_hook(webui_shared, device_index, "UpscalerDAT")


def install_hat_hook(webui_shared, device_index: int = 0):
    """Point the webui's HAT scaler objects (modules/hat_model.py: the HAT files found in the model directory, loaded there through
    spandrel) at the engine: install_swinir_hook for the entries of ``webui_shared.sd_upscalers`` whose scaler class is UpscalerHAT.
    ``do_upscale(img, path)`` runs the checkpoint as sdmi_hat_run on the image whole instead of as a torch module in HAT_tile tiles.  The
    same fall-back rules: a URL that is not on disk yet, a checkpoint the loader refuses (another window size or overlap ratio, head dim
    > 32, 3conv groups, pixelshuffledirect or no upsampler, num_feat other than 64, a grey-scale model, an index buffer that is not a
    function of the key offset) or that fails to load or pack, and an image too large for the arena or with a side below 9 stay on the
    stock path.  Idempotent.  Returns the names of the hooked entries."""
    return _install_whole_image_hook(webui_shared, device_index, "UpscalerHAT")


def _install_whole_image_hook(webui_shared, device_index, scaler_class):
    from . import upscaler as amd_upscaler
    engine_scaler = amd_upscaler.UpscalerESRGAN(device_index)
    hooked = []
    for data in getattr(webui_shared, "sd_upscalers", []):
        scaler = getattr(data, "scaler", None)
        if scaler is None or type(scaler).__name__ != scaler_class:
            continue
        hooked.append(data.name)
        if hasattr(scaler.do_upscale, "_mi355x_stock"):
            continue
        stock = scaler.do_upscale

        def do_upscale(img, model_file=None, _stock=stock, _scaler=scaler):
            path = model_file
            info = next((d for d in getattr(_scaler, "scalers", []) if model_file in (d.data_path, d.name)), None)
            if info is not None:
                path = getattr(info, "local_data_path", None) or info.data_path
            if not isinstance(path, str) or path.startswith("http"):
                return _stock(img, model_file)                    # not on disk yet: the stock code downloads (and runs) it
            try:
                engine_scaler.load_model(path)
            except Exception:                                     # the loader's refusal (ValueError), an unreadable file, an engine error
                return _stock(img, model_file)
            try:
                return engine_scaler.do_upscale(img, path)
            except ValueError:                                    # EsrganInputTooLarge (the stock path tiles it), or a side below one window
                return _stock(img, model_file)
        do_upscale._mi355x_stock = stock
        scaler.do_upscale = do_upscale
    return hooked
