"""On-disk format of a compressed model — interoperable with the reference's exported repos.

The reference's exporter (huggingface_repos/build_asvd_repo.py:58-92) writes an ordinary `save_pretrained` checkpoint whose
factorised layers appear under the state-dict keys `<layer>.ALinear.weight` / `.ALinear.bias` / `<layer>.BLinear.weight`,
plus `config.json` extended with
    "truncation_ranks": {<layer full name>: rank},  "auto_map": {...},  "architectures": ["ASVD<Family>ForCausalLM"]
and a pair of remote-code files whose model class rebuilds the two-Linear modules from `truncation_ranks` before the weights
are loaded (huggingface_repos/modeling_asvd_llama.py:5-41).  `save_asvd_repo` writes exactly that layout; the loader files
it emits are generated from the templates below (subclassing the stock HF config/model classes), so the directory loads
with `AutoModelForCausalLM.from_pretrained(path, trust_remote_code=True)` as the published `hahnyuan/*-asvd*` repos do.
`load_asvd_repo` is a family-agnostic loader that needs no remote code; it also reads repos exported by the reference.

A model whose weights were packed (`--weight_quant_storage packed`: W8Linear modules) is written as it is — the checkpoint then holds
`<layer>.qweight` (uint8), `.scales`, `.zeros` (fp32) in place of `<layer>.weight` — with `"weight_quant": {"method": "rtn", "bits": b,
"storage": "uint8"}` in config.json and WITHOUT `auto_map` and the remote-code files, which cannot rebuild packed modules: such a repo loads
with `load_asvd_repo` only.  A model whose codes are stored at their own width (`--weight_quant_storage bitpacked`: WBLinear modules) is written
the same way with `<layer>.qbits` (uint8 bitstream rows, modules/wb_linear.py) in place of `.qweight` and `"storage": "bitstream64"`.  One
model holds one width and one storage form.  Group-wise scales (`--weight_quant_group_size G`) add `"group_size": G` to `weight_quant` and
make `.scales` / `.zeros` [out, ceil(in / G)]; the key is absent for per-row scales, and one model holds one group size.  The clip search (`--weight_quant_mse`) changes nothing on disk: it
only gives `.scales` / `.zeros` other values, so the format has no key for it and a loaded model does not know whether its pairs were searched.
"""
import json
import os

import torch
import torch.nn as nn

from .modules.svd_linear import SVDLinear
from .modules.w8_linear import W8Linear, param_shape
from .modules.wb_linear import WBLinear, row_bytes

_FAMILIES = {
    # family tag -> (HF config class, HF model class, file stem)
    "llama": ("LlamaConfig", "LlamaForCausalLM", "llama"),
    "opt": ("OPTConfig", "OPTForCausalLM", "opt"),
}

_CONFIG_TEMPLATE = '''"""Config of an ASVD-compressed {cls_model}: the stock config plus `truncation_ranks` ({{layer name: rank}})."""
from transformers import {cls_config}


class ASVD{Fam}Config({cls_config}):
    model_type = "{model_type}"

    def __init__(self, truncation_ranks=None, **kwargs):
        super().__init__(**kwargs)
        self.truncation_ranks = truncation_ranks if truncation_ranks is not None else {{}}
'''

_MODELING_TEMPLATE = '''"""ASVD-compressed {cls_model}: every layer named in config.truncation_ranks is a pair BLinear (in -> r, no bias),
ALinear (r -> out, original bias) — the module/key names of ASVD4LLM's SVDLinear."""
import torch.nn as nn
from transformers import {cls_model}

from .configuration_asvd_{stem} import ASVD{Fam}Config


class ASVDLinear(nn.Module):
    def __init__(self, in_features, out_features, rank, bias=True):
        super().__init__()
        self.BLinear = nn.Linear(in_features, rank, bias=False)
        self.ALinear = nn.Linear(rank, out_features, bias=bias)
        self.truncation_rank = rank

    def forward(self, x):
        return self.ALinear(self.BLinear(x))


class ASVD{Fam}ForCausalLM({cls_model}):
    config_class = ASVD{Fam}Config

    def __init__(self, config):
        super().__init__(config)
        self.truncation_ranks = dict(config.truncation_ranks or {{}})
        for full_name, rank in self.truncation_ranks.items():
            parent_name, _, child = full_name.rpartition(".")
            parent = self.get_submodule(parent_name) if parent_name else self
            lin = getattr(parent, child)
            setattr(parent, child, ASVDLinear(lin.in_features, lin.out_features, int(rank), bias=lin.bias is not None))
'''


def _family_of(model_or_config):
    cfg = getattr(model_or_config, "config", model_or_config)
    mt = getattr(cfg, "model_type", "")
    for fam in _FAMILIES:
        if fam in mt:
            return fam
    raise ValueError(f"no ASVD repo template for model_type={mt!r} (supported: {sorted(_FAMILIES)})")


def truncation_ranks_of(model):
    """{full layer name: rank} of every SVDLinear, in named_modules order (build_asvd_repo.py:66-69)."""
    return {name: int(m.truncation_rank) for name, m in model.named_modules() if isinstance(m, SVDLinear)}


def replace_with_factor_pairs(model, truncation_ranks, dtype=None):
    """Swap each named nn.Linear for an (uninitialised) SVDLinear-shaped module so a checkpoint with ALinear/BLinear keys fits."""
    for full_name, rank in truncation_ranks.items():
        parent_name, _, child = full_name.rpartition(".")
        parent = model.get_submodule(parent_name) if parent_name else model
        lin = getattr(parent, child)
        if not isinstance(lin, nn.Linear):
            raise ValueError(f"{full_name} is not an nn.Linear in the base architecture")
        dt = dtype or lin.weight.dtype
        A = torch.empty(lin.out_features, int(rank), dtype=dt, device=lin.weight.device)
        B = torch.empty(int(rank), lin.in_features, dtype=dt, device=lin.weight.device)
        bias = torch.empty(lin.out_features, dtype=dt, device=lin.weight.device) if lin.bias is not None else None
        setattr(parent, child, SVDLinear._from_factors(A, B, bias, int(rank)))
    return model


def packed_layers_of(model):
    """{full layer name: bits} of every W8Linear, in named_modules order"""
    return {name: int(m.bits) for name, m in model.named_modules() if isinstance(m, W8Linear)}


def bitpacked_layers_of(model):
    """{full layer name: bits} of every WBLinear, in named_modules order"""
    return {name: int(m.bits) for name, m in model.named_modules() if isinstance(m, WBLinear)}


def group_sizes_of(model):
    """the set of group sizes (0: per row) of the packed layers of the model"""
    return {int(getattr(m, "group_size", 0)) for m in model.modules() if isinstance(m, (W8Linear, WBLinear))}


def _check_param_shapes(state, full_name, out_f, in_f, group_size):
    """the checkpoint's scales / zeros of a packed layer must have the shape the group size gives them"""
    want = param_shape(out_f, in_f, group_size)
    for key in ("scales", "zeros"):
        have = state.get(f"{full_name}.{key}")
        if have is not None and tuple(have.shape) != want:
            raise ValueError(f"{full_name}.{key} is {tuple(have.shape)} in the checkpoint, but weight_quant.group_size={group_size} makes it "
                             f"{want} for a [{out_f}, {in_f}] weight")


def replace_with_bitpacked(model, state, bits, dtype=None, group_size=0):
    """Swap every module whose checkpoint keys end in `.qbits` for an empty WBLinear.  in_features comes from the module that is there (the base
    architecture's Linear, or the factor pair built from truncation_ranks); the checkpoint's rows must be the bitstream of that many codes."""
    for key in [k for k in state if k.endswith(".qbits")]:
        full_name = key[: -len(".qbits")]
        parent_name, _, child = full_name.rpartition(".")
        parent = model.get_submodule(parent_name) if parent_name else model
        old = getattr(parent, child)
        if not isinstance(old, nn.Linear) or tuple(state[key].shape) != (old.out_features, row_bytes(old.in_features, bits)):
            raise ValueError(f"{full_name}: bit-packed weight {tuple(state[key].shape)} ({bits} bits) does not fit {old}")
        _check_param_shapes(state, full_name, old.out_features, old.in_features, group_size)
        setattr(parent, child, WBLinear(old.in_features, old.out_features, bias=old.bias is not None, bits=bits, weight_dtype=dtype or old.weight.dtype,
                                        device=old.weight.device, group_size=group_size))
    return model


def replace_with_packed(model, state, bits=8, dtype=None, group_size=0):
    """Swap every module whose checkpoint keys end in `.qweight` for an empty W8Linear of the checkpoint's shape, so that the packed keys fit."""
    for key in [k for k in state if k.endswith(".qweight")]:
        full_name = key[: -len(".qweight")]
        parent_name, _, child = full_name.rpartition(".")
        parent = model.get_submodule(parent_name) if parent_name else model
        old = getattr(parent, child)
        out_f, in_f = state[key].shape
        if not isinstance(old, nn.Linear) or (old.out_features, old.in_features) != (out_f, in_f):
            raise ValueError(f"{full_name}: packed weight {tuple(state[key].shape)} does not fit {old}")
        _check_param_shapes(state, full_name, out_f, in_f, group_size)
        setattr(parent, child, W8Linear(in_f, out_f, bias=old.bias is not None, bits=bits, weight_dtype=dtype or old.weight.dtype,
                                        device=old.weight.device, group_size=group_size))
    return model


def save_asvd_repo(model, save_path, tokenizer=None, family=None):
    """Write `save_path/` in the reference's exported-repo layout.  Returns the truncation_ranks dict.  A model with packed weights
    (W8Linear) gets `weight_quant` in config.json and no remote-code loader (see the module docstring)."""
    fam = family or _family_of(model)
    cls_config, cls_model, stem = _FAMILIES[fam]
    Fam = {"llama": "Llama", "opt": "OPT"}[fam]
    os.makedirs(save_path, exist_ok=True)
    if tokenizer is not None:
        tokenizer.save_pretrained(save_path)
    model.save_pretrained(save_path)
    config = model.config.to_dict()
    ranks = truncation_ranks_of(model)
    config["truncation_ranks"] = ranks
    packed, bitpacked = packed_layers_of(model), bitpacked_layers_of(model)
    if packed and bitpacked:
        raise ValueError(f"{len(packed)} uint8-packed next to {len(bitpacked)} bit-packed layers: one model holds one storage form")
    if packed or bitpacked:
        storage = "uint8" if packed else "bitstream64"
        packed = packed or bitpacked
        if len(set(packed.values())) != 1:
            raise ValueError(f"packed layers of several bit widths in one model: {sorted(set(packed.values()))}")
        groups = group_sizes_of(model)
        if len(groups) != 1:
            raise ValueError(f"packed layers of several group sizes in one model: {sorted(groups)}")
        config["weight_quant"] = {"method": "rtn", "bits": next(iter(packed.values())), "storage": storage}
        if next(iter(groups)):
            config["weight_quant"]["group_size"] = next(iter(groups))
        config.pop("auto_map", None)
        with open(os.path.join(save_path, "config.json"), "w") as f:
            json.dump(config, f, indent=2)
        print(f"{len(packed)} packed ({storage}) weights: no auto_map / remote-code files written, load with asvd4llm_amd.export.load_asvd_repo")
        return ranks
    config["auto_map"] = {
        "AutoConfig": f"configuration_asvd_{stem}.ASVD{Fam}Config",
        "AutoModelForCausalLM": f"modeling_asvd_{stem}.ASVD{Fam}ForCausalLM",
    }
    config["architectures"] = [f"ASVD{Fam}ForCausalLM"]
    fmt = dict(cls_config=cls_config, cls_model=cls_model, stem=stem, Fam=Fam, model_type=config.get("model_type", fam))
    with open(os.path.join(save_path, f"configuration_asvd_{stem}.py"), "w") as f:
        f.write(_CONFIG_TEMPLATE.format(**fmt))
    with open(os.path.join(save_path, f"modeling_asvd_{stem}.py"), "w") as f:
        f.write(_MODELING_TEMPLATE.format(**fmt))
    with open(os.path.join(save_path, "config.json"), "w") as f:
        json.dump(config, f, indent=2)
    return ranks


def _read_state_dict(path):
    st = {}
    files = sorted(f for f in os.listdir(path) if f.endswith(".safetensors"))
    if files:
        from safetensors.torch import load_file
        for f in files:
            st.update(load_file(os.path.join(path, f)))
        return st
    files = sorted(f for f in os.listdir(path) if f.endswith(".bin") and f.startswith("pytorch_model"))
    for f in files:
        st.update(torch.load(os.path.join(path, f), map_location="cpu"))
    if not st:
        raise FileNotFoundError(f"no weights (*.safetensors / pytorch_model*.bin) under {path}")
    return st


def load_asvd_repo(path, dtype=torch.float16, device="cpu"):
    """Load an exported ASVD repo (ours or the reference's) without remote code: stock architecture from config.json,
    factor pairs from `truncation_ranks`, then the checkpoint (strict, except tied / re-creatable buffers)."""
    from transformers import AutoConfig, AutoModelForCausalLM
    with open(os.path.join(path, "config.json")) as f:
        raw = json.load(f)
    ranks = raw.pop("truncation_ranks", {}) or {}
    raw.pop("auto_map", None)
    fam = next((k for k in _FAMILIES if k in raw.get("model_type", "")), None)
    if fam is None:
        raise ValueError(f"unsupported model_type {raw.get('model_type')!r}")
    raw["architectures"] = [_FAMILIES[fam][1]]
    cfg = AutoConfig.for_model(**raw)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        model = AutoModelForCausalLM.from_config(cfg)
    finally:
        torch.set_default_dtype(prev)
    replace_with_factor_pairs(model, ranks, dtype=dtype)
    state = _read_state_dict(path)
    wq = raw.get("weight_quant") or {}
    if any(k.endswith((".qweight", ".qbits")) for k in state):
        # the codes stand for weights of ONE dtype, the model's at pack time (save_pretrained records it); loading them as another would
        # round every weight once more and take the packed layers off the kernel path
        packed_dtype = raw.get("torch_dtype") or raw.get("dtype")
        if packed_dtype is not None and getattr(torch, str(packed_dtype), None) != dtype:
            raise ValueError(f"{path} holds weights packed from {packed_dtype}; load it with dtype=torch.{packed_dtype} (got {dtype})")
        group_size = int(wq.get("group_size", 0))
        if group_size not in (0, 64, 128):
            raise ValueError(f"{path}: weight_quant.group_size must be 64 or 128 when present (got {group_size})")
        replace_with_packed(model, state, bits=int(wq.get("bits", 8)), dtype=dtype, group_size=group_size)
        if any(k.endswith(".qbits") for k in state):
            if "bits" not in wq:
                raise ValueError(f"{path} holds bit-packed weights but config.json does not give their width (weight_quant.bits)")
            replace_with_bitpacked(model, state, bits=int(wq["bits"]), dtype=dtype, group_size=group_size)
    missing, unexpected = model.load_state_dict(state, strict=False)
    tied_ok = {"lm_head.weight"} if getattr(cfg, "tie_word_embeddings", False) else set()
    bad_missing = [k for k in missing if k not in tied_ok and not k.endswith("rotary_emb.inv_freq")]
    if bad_missing or unexpected:
        raise RuntimeError(f"checkpoint does not match truncation_ranks: missing={bad_missing[:5]} unexpected={list(unexpected)[:5]}")
    if tied_ok and "lm_head.weight" in missing:
        model.tie_weights()
    model.truncation_ranks = ranks
    return model.to(device).eval()
