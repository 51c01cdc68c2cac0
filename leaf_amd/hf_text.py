"""The engine's text tower behind HuggingFace's ``CLIPTextModel`` / ``CLIPTextModelWithProjection`` call surface.

The reference ships its robust text encoders in that format and puts them into a diffusion pipeline as ``pipeline.text_encoder`` /
``text_encoder_2`` (eval_text_to_image.py:172-178); its attack wrappers read ``self(x).pooler_output`` / ``.text_embeds``
(utils_attacks.py:49-59).  ``LeafHFTextEncoder`` is the callable those consumers touch, computed by ``encode_text_hidden``:

    pipeline.text_encoder = LeafHFTextEncoder(model)                              # SD 1.x / 2.x, SDXL's first encoder
    pipeline.text_encoder_2 = LeafHFTextEncoder(model_2, with_projection=True)    # SDXL's second encoder

It uses three names of the model -- ``encode_text_hidden``, ``encode_text`` and ``cfg`` (plus ``device`` when the model has one) --
so its wiring is checked on the CPU against a stub (tests/test_hidden_cpu.py).  No attention masks: CLIP pipelines pass none, and
the tower is causal.  Forward only: the states carry no autograd graph."""
from types import SimpleNamespace

import torch


class TextEncoderOutput:
    """``last_hidden_state`` [N, ctx, width], ``pooler_output`` (plain) or ``text_embeds`` (with projection), ``hidden_states`` (a tuple of
    layers + 1 tensors, or None); as a tuple: HF's order with the None entries dropped."""

    def __init__(self, last_hidden_state, pooler_output=None, text_embeds=None, hidden_states=None):
        self.last_hidden_state, self.pooler_output, self.text_embeds, self.hidden_states = last_hidden_state, pooler_output, text_embeds, hidden_states

    def to_tuple(self):
        # CLIPTextModelOutput: (text_embeds, last_hidden_state, hidden_states); BaseModelOutputWithPooling: (last_hidden_state, pooler_output, hidden_states)
        order = (self.text_embeds, self.last_hidden_state) if self.text_embeds is not None else (self.last_hidden_state, self.pooler_output)
        return tuple(x for x in order + (self.hidden_states,) if x is not None)

    def __getitem__(self, i):
        return self.to_tuple()[i]


class LeafHFTextEncoder:
    def __init__(self, model, with_projection: bool = False):
        self.model = model
        self.with_projection = bool(with_projection)
        cfg = model.cfg
        self.config = SimpleNamespace(hidden_size=cfg.width, projection_dim=cfg.embed_dim, num_hidden_layers=cfg.layers,
                                      max_position_embeddings=cfg.context_length)
        self.dtype = torch.float32
        self.device = getattr(model, "device", torch.device("cpu"))

    def encode_text(self, x, normalize: bool = False):
        """the reference's ``encode_text_wrapper`` / ``_2`` (utils_attacks.py:49-59) without the detour: the engine's features"""
        return self.model.encode_text(x, normalize=normalize)

    def __call__(self, input_ids, attention_mask=None, output_hidden_states=False, **ignored_none_kwargs):
        if attention_mask is not None:
            raise ValueError("LeafHFTextEncoder takes no attention_mask: the tower is causal and CLIP pipelines pass none")
        given = sorted(k for k, v in ignored_none_kwargs.items() if v is not None)
        if given:
            raise TypeError(f"LeafHFTextEncoder: unsupported arguments {given}")
        L = self.model.cfg.layers
        if output_hidden_states:      # every entry of hidden_states (no ln_final) + last_hidden_state = ln_final of the last one
            layers, lns = list(range(L + 1)) + [L], [False] * (L + 1) + [True]
        else:
            layers, lns = [L], [True]
        # all ctx rows: a pipeline cross-attends to the padded positions too
        got = self.model.encode_text_hidden(input_ids, layers=layers, final_ln=lns, seq_lens="dense", want_features=self.with_projection)
        states, feat = got if self.with_projection else (got, None)
        last = states[-1]
        out = TextEncoderOutput(last, hidden_states=tuple(states[:-1]) if output_hidden_states else None)
        if self.with_projection:
            out.text_embeds = feat
        else:
            # the row at the FIRST maximum id: the engine's pooling (= HF's for well-formed ids; torch.argmax returns the first maximum)
            ids = torch.as_tensor(input_ids).to(last.device)
            out.pooler_output = last[torch.arange(last.shape[0], device=last.device), ids.long().argmax(-1)]
        return out
