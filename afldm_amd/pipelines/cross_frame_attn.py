"""Cross-frame ("equivariant") attention hook — surface of reference
afldm/pipelines/cross_frame_attn.py (AttnState :6-51, CrossFrameAttnProcessor :54-130,
get_/set_unet_attn_processor :133-190) over afldm_amd's Attention modules.

STORE: remember the pre-norm input of every self-attention, keyed by timestep; LOAD: take K and
V from the remembered (unshifted-pass) map, group-normed with the layer's own GroupNorm, while
Q comes from the current hidden states.  Tensors are NHWC inside the UNet forward."""
import torch

from .. import ops
from ..models.blocks import AttnProcessor2_0, packed_norm


class AttnState:
    """What the cross-frame processors of one UNet share (API of the reference's AttnState, cross_frame_attn.py:6-51):
    the mode - STORE the attention inputs of this pass / LOAD the stored ones as K, V / IDLE - plus the timestep that keys
    the stored maps, the slot a STORE pass writes (`store_id`, two slots for the interpolating processor) and the blend
    weight `alpha` of a LOAD pass.  `state`, `timestep`, `store_id` and `alpha` are read-only views; they change through
    the set_* / to_* methods only, exactly as in the reference.

    Beyond the reference: `set_store_id(AttnState.PAIR)` makes ONE batch-2 STORE pass fill both slots (sample 0 -> slot 0, sample
    1 -> slot 1: the samples are independent, so this is the reference's two batch-1 passes at half the launches), and
    `set_alpha` also takes a 1-D fp32 device tensor, one blend weight per sample of the LOAD batch.
    `set_store_id(AttnState.BANK)` makes a STORE pass at ANY batch S keep the whole batch as one bank of S sources per timestep,
    and `set_sources(t)` - t an int32 [B, 2] tensor - names, per sample of a LOAD batch, the two bank slots it attends to (the
    banked processor, enable_bank; blended by that sample's alpha)."""
    STORE, LOAD, IDLE = 0, 1, 2
    PAIR = -1
    BANK = -2
    _FIELDS = ("state", "timestep", "store_id", "alpha", "sources")

    def __init__(self):
        self._v = {}
        self.reset()

    def reset(self):
        self._v.update(state=self.STORE, timestep=0, store_id=0, alpha=0, sources=None)

    def __getattr__(self, name):                      # only reached for names that are not real attributes
        if name in AttnState._FIELDS:
            return self.__dict__["_v"][name]
        raise AttributeError(name)

    def __setattr__(self, name, value):
        if name in AttnState._FIELDS:
            raise AttributeError(f"AttnState.{name} is read-only: use set_{name}() / to_load() / to_idle() / reset()")
        object.__setattr__(self, name, value)

    def set_timestep(self, t):
        self._v["timestep"] = t.item() if torch.is_tensor(t) else t

    def set_alpha(self, alpha):
        """A float (the reference: one weight for the whole LOAD batch) or a 1-D fp32 tensor of one weight per sample, on the
        device for the cached path (afldm_attention_interp reads it when the kernel runs: a captured graph sees the values the
        tensor holds at each replay)."""
        if torch.is_tensor(alpha) and (alpha.ndim != 1 or alpha.dtype != torch.float32):
            raise ValueError(f"AttnState.set_alpha: a tensor alpha must be 1-D fp32 (one weight per sample), got "
                             f"{alpha.dtype} {tuple(alpha.shape)}")
        self._v["alpha"] = alpha

    def set_sources(self, sources):
        """int32 [B, 2]: sample b of the LOAD batch attends to bank slots sources[b] = (s0, s1).  On the device for the cached
        path (afldm_attention_bank reads it when the kernel runs, and clamps it into the bank); None clears it."""
        if sources is not None and not (torch.is_tensor(sources) and sources.ndim == 2 and sources.shape[1] == 2
                                        and sources.dtype == torch.int32):
            what = f"{sources.dtype} {tuple(sources.shape)}" if torch.is_tensor(sources) else type(sources).__name__
            raise ValueError(f"AttnState.set_sources: sources must be an int32 tensor [B, 2], got {what}")
        self._v["sources"] = sources

    def set_store_id(self, store_id):
        self._v["store_id"] = store_id

    def to_load(self):
        self._v["state"] = self.LOAD

    def to_idle(self):
        self._v["state"] = self.IDLE


class CrossFrameAttnProcessor(AttnProcessor2_0):
    """cache_kv (not in the reference; the graph-replayed harness sets it): a STORE pass also keeps the keys / values it
    projects from its own hidden states, and a LOAD pass attends to them directly instead of group-norming and projecting the
    stored map again every step (reference cross_frame_attn.py:88-125 recomputes them: same layer, same input, same numbers).
    `maps` is still filled as the reference does.  With enable_interp, a LOAD pass that finds both slots cached runs
    to_q -> ONE afldm_attention_interp launch over both stored pairs (per-sample alpha) -> ONE to_out + residual, instead of
    two GroupNorms, two K / V projections, two attentions, two to_out GEMMs and a torch blend.
    enable_bank (frame sequences, LDMVideoPipeline): a STORE pass with store_id BANK keeps its whole batch of S samples in slot
    0 as one bank, and a LOAD pass lets sample b attend to bank slots attn_state.sources[b] = (s0, s1), blended by its alpha.
    With cached K / V that is to_q -> ONE afldm_attention_bank launch -> ONE to_out + residual; without, the eager yardstick:
    per sample and named source one GroupNorm + K / V projection of that slot's stored map and one afldm_attention, then the
    torch blend (a sample whose alpha is 0 runs its first source only, like the kernel)."""

    def __init__(self, attn_state: AttnState, enable_interp=False, cache_kv=False, enable_bank=False):
        super().__init__()
        self.attn_state = attn_state
        self.maps = [dict(), dict()]
        self.kv = [dict(), dict()]
        self.enable_interp = enable_interp
        self.cache_kv = bool(cache_kv)
        self.enable_bank = bool(enable_bank)
        if self.enable_bank and self.enable_interp:
            raise ValueError("CrossFrameAttnProcessor: enable_bank and enable_interp are two different LOAD modes")

    def _load_bank(self, attn, hidden_states, attention_mask, temb, t):
        """LOAD of the banked processor (see the class docstring)."""
        B = hidden_states.shape[0]
        src = self.attn_state.sources
        if src is None or src.shape[0] != B:
            raise ValueError(f"a banked LOAD pass of {B} samples needs AttnState.set_sources with an int32 [{B}, 2] tensor, got "
                             f"{None if src is None else tuple(src.shape)}")
        if self.cache_kv and t in self.kv[0]:
            if src.device != hidden_states.device:
                raise ValueError(f"sources on {src.device} do not match the LOAD batch on {hidden_states.device}")
            return AttnProcessor2_0.__call__(self, attn, hidden_states, None, attention_mask, temb, kv=self.kv[0][t], src=src,
                                             alpha=self._alpha_vector(B, hidden_states.device))
        bank = self.maps[0][t]
        S = bank.shape[0]
        alpha = self.attn_state.alpha
        alphas = [float(a) for a in alpha.tolist()] if torch.is_tensor(alpha) else [float(alpha)] * B
        if len(alphas) != B:
            raise ValueError(f"per-sample alpha of {len(alphas)} weights does not match the LOAD batch {B}")
        rows = []
        for b, (s0, s1) in enumerate(src.tolist()):
            x = hidden_states[b:b + 1]
            per = []
            for s in (s0, s1) if alphas[b] != 0.0 else (s0,):
                s = min(max(s, 0), S - 1)
                per.append(AttnProcessor2_0.__call__(self, attn, x, self._kv_source(attn, bank[s:s + 1], 1), attention_mask, temb))
            rows.append(per[0] if len(per) == 1 else (1 - alphas[b]) * per[0] + alphas[b] * per[1])
        return torch.cat(rows) if B > 1 else rows[0]

    def _alpha_vector(self, batch, device):
        """The LOAD pass's blend weights as the fp32 device vector [batch] the interpolating kernel reads."""
        alpha = self.attn_state.alpha
        if torch.is_tensor(alpha):
            if tuple(alpha.shape) != (batch,) or alpha.device != device:
                raise ValueError(f"per-sample alpha {tuple(alpha.shape)} on {alpha.device} does not match the LOAD batch "
                                 f"{batch} on {device}")
            return alpha
        return torch.full((batch,), float(alpha), dtype=torch.float32, device=device)

    def _kv_source(self, attn, stored, batch):
        """group-normed [Bk, HW, C] tokens of a stored NHWC map; Bk must divide the batch (the
        kernel indexes kv-sample b // (B/Bk): the reference's batch repeat, cross_frame_attn.py:91-96)."""
        Bk, H, W, C = stored.shape
        if batch % Bk != 0:
            raise ValueError(f"stored map batch {Bk} does not divide the current batch {batch}")
        gn = attn.group_norm
        if gn is None:
            return stored.view(Bk, H * W, C)
        gamma, beta = packed_norm(gn)
        stats = ops.gn_stats(stored, gn.num_groups)
        return ops.gn_apply(stored, stats, gamma, beta, gn.num_groups, gn.eps, act=0).view(Bk, H * W, C)

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None):
        if encoder_hidden_states is not None:       # not self-attention: vanilla
            return super().__call__(attn, hidden_states, encoder_hidden_states, attention_mask, temb)
        st, t = self.attn_state.state, self.attn_state.timestep
        if st == AttnState.IDLE:
            return super().__call__(attn, hidden_states, None, attention_mask, temb)
        if st == AttnState.STORE:
            sid = self.attn_state.store_id
            # (under graph capture the tensor lives in the graph's pool for as long as this dict holds it and nobody writes it
            #  in place: no copy launch; eager passes keep the reference's clone)
            capturing = torch.cuda.is_current_stream_capturing()
            if sid == AttnState.PAIR:
                return self._store_pair(attn, hidden_states, attention_mask, temb, t, capturing)
            if sid == AttnState.BANK:             # the whole batch, as one bank of S sources, in slot 0
                sid = 0
            self.maps[sid][t] = hidden_states.detach() if capturing else hidden_states.detach().clone()
            if not self.cache_kv:
                return super().__call__(attn, hidden_states, None, attention_mask, temb)
            return super().__call__(attn, hidden_states, None, attention_mask, temb,
                                    kv_sink=lambda k, vt: self.kv[sid].__setitem__(t, (k, vt)))
        if self.enable_bank:
            return self._load_bank(attn, hidden_states, attention_mask, temb, t)
        B = hidden_states.shape[0]
        if self.cache_kv and t in self.kv[0] and B % self.kv[0][t][0].shape[0] == 0:
            if not self.enable_interp:
                return super().__call__(attn, hidden_states, None, attention_mask, temb, kv=self.kv[0][t])
            if t in self.kv[1] and self.kv[1][t][0].shape == self.kv[0][t][0].shape:
                return super().__call__(attn, hidden_states, None, attention_mask, temb, kv=self.kv[0][t], kv1=self.kv[1][t],
                                        alpha=self._alpha_vector(B, hidden_states.device))
        map0 = self._kv_source(attn, self.maps[0][t], hidden_states.shape[0])
        if not self.enable_interp:
            return super().__call__(attn, hidden_states, map0, attention_mask, temb)
        alpha = self.attn_state.alpha
        map1 = self._kv_source(attn, self.maps[1][t], hidden_states.shape[0])
        r1 = super().__call__(attn, hidden_states, map0, attention_mask, temb)
        r2 = super().__call__(attn, hidden_states, map1, attention_mask, temb)
        if torch.is_tensor(alpha):                  # one weight per sample (NHWC: broadcast over H, W, C)
            alpha = alpha.to(device=r1.device, dtype=r1.dtype).view(-1, 1, 1, 1)
        return (1 - alpha) * r1 + alpha * r2

    def _store_pair(self, attn, hidden_states, attention_mask, temb, t, capturing):
        """STORE with store_id PAIR: one batch-2 pass fills both slots, sample s -> slot s, as [s:s+1] views of the same maps /
        K / V^T buffers."""
        if hidden_states.shape[0] != 2:
            raise ValueError(f"a two-slot STORE pass (store_id PAIR) runs at batch 2, got {hidden_states.shape[0]}")
        for s in (0, 1):
            m = hidden_states[s:s + 1].detach()
            self.maps[s][t] = m if capturing else m.clone()
        if not self.cache_kv:
            return super().__call__(attn, hidden_states, None, attention_mask, temb)

        def sink(k, vt):
            for s in (0, 1):
                self.kv[s][t] = (k[s:s + 1], vt[s:s + 1])
        return super().__call__(attn, hidden_states, None, attention_mask, temb, kv_sink=sink)


def get_unet_attn_processors(unet):
    """{'<module path>.processor': processor} for every module exposing get_processor()."""
    found = {}

    def walk(name, module):
        if hasattr(module, "get_processor"):
            found[f"{name}.processor"] = module.get_processor()
        for sub, child in module.named_children():
            walk(f"{name}.{sub}", child)

    for name, module in unet.named_children():
        walk(name, module)
    return found


def set_unet_attn_processor(unet, processor):
    count = len(get_unet_attn_processors(unet))
    if isinstance(processor, dict) and len(processor) != count:
        raise ValueError(
            f"A dict of processors was passed, but the number of processors {len(processor)} does not match the"
            f" number of attention layers: {count}. Please make sure to pass {count} processor classes.")

    def walk(name, module):
        if hasattr(module, "set_processor"):
            module.set_processor(processor.pop(f"{name}.processor") if isinstance(processor, dict) else processor)
        for sub, child in module.named_children():
            walk(f"{name}.{sub}", child)

    for name, module in unet.named_children():
        walk(name, module)


def eager_pass(model, scheduler, attn_state, timesteps, latents, step_fn):
    """`timesteps` eagerly, as the reference's loops run a STORE or LOAD pass: attn_state.set_timestep(t), eps = model(x, t)
    - the UNet, or whatever evaluates it on the (scaled) latents - then latents = step_fn(eps, t, latents)."""
    for t in timesteps:
        attn_state.set_timestep(t)
        latents = step_fn(model(scheduler.scale_model_input(latents, t), t), t, latents)
    return latents
