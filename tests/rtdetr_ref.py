"""Tests-side reference of Ultralytics RT-DETR-l (rtdetr-l.yaml) in eval mode: a torch-CPU restatement, in fp64 or fp32, of the
modules and functions of Ultralytics 8.x that the model runs, written from the library's definitions (Ultralytics is not installed
here): nn/modules/block.py HGStem, HGBlock, RepC3; nn/modules/conv.py Conv, LightConv, DWConv, RepConv; nn/modules/transformer.py
TransformerEncoderLayer, AIFI (build_2d_sincos_position_embedding), MSDeformAttn, DeformableTransformerDecoderLayer; nn/modules/utils.py
multi_scale_deformable_attn_pytorch, inverse_sigmoid; nn/modules/head.py RTDETRDecoder (_generate_anchors, _get_encoder_input,
_get_decoder_input, the decoder loop with eval_idx = -1); models/rtdetr/predict.py RTDETRPredictor (pre_transform, postprocess).

It reads either the unfused state dict (synth.rtdetr_l_state_dict: BatchNorm applied as a module with eps 1e-3, RepConv as its two
branches, nn.MultiheadAttention's packed in_proj) or the converted FFPW tensors (folded convs, one 3x3 per RepConv, split q/k/v).
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle.ultra_post import resize_linear_u8

HGBLOCKS = [(1, 48, 48, 128, 3, False, False), (3, 128, 96, 512, 3, False, False), (5, 512, 192, 1024, 5, True, False),
            (6, 1024, 192, 1024, 5, True, True), (7, 1024, 192, 1024, 5, True, True), (9, 1024, 384, 2048, 5, True, False)]
HD, NQ, NH, NL, NP = 256, 300, 8, 3, 4
BN_EPS = 1e-3


class Ref:
    def __init__(self, sd: dict, dtype=torch.float64):
        self.dt = dtype
        self.sd = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd.items()}
        self.nc = int(self.sd["model.28.enc_score_head.weight"].shape[0])

    def t(self, k):
        return self.sd[k]

    # ---- nn/modules/conv.py ----
    def conv(self, p, x, s=1, pad=None, g=1, act=None):
        w = self.t(p + ".conv.weight")
        k = w.shape[-1]
        pad = k // 2 if pad is None else pad
        if p + ".bn.weight" in self.sd:
            y = F.conv2d(x, w, None, s, pad, 1, g)
            y = F.batch_norm(y, self.t(p + ".bn.running_mean"), self.t(p + ".bn.running_var"), self.t(p + ".bn.weight"), self.t(p + ".bn.bias"),
                             False, 0.0, BN_EPS)
        else:
            y = F.conv2d(x, w, self.t(p + ".conv.bias"), s, pad, 1, g)
        return act(y) if act is not None else y

    def repconv(self, p, x):
        if p + ".conv1.conv.weight" in self.sd:
            return F.silu(self.conv(p + ".conv1", x, pad=1) + self.conv(p + ".conv2", x, pad=0))
        return self.conv(p, x, act=F.silu)

    def lightconv(self, p, x, k):
        y = self.conv(p + ".conv1", x)
        return self.conv(p + ".conv2", y, g=y.shape[1], act=F.relu)

    # ---- nn/modules/block.py ----
    def hgstem(self, x):
        x = self.conv("model.0.stem1", x, 2, act=F.relu)
        x = F.pad(x, [0, 1, 0, 1])
        x2 = self.conv("model.0.stem2a", x, 1, 0, act=F.relu)
        x2 = F.pad(x2, [0, 1, 0, 1])
        x2 = self.conv("model.0.stem2b", x2, 1, 0, act=F.relu)
        x1 = F.max_pool2d(x, 2, 1, 0, ceil_mode=True)
        x = torch.cat([x1, x2], 1)
        x = self.conv("model.0.stem3", x, 2, act=F.relu)
        return self.conv("model.0.stem4", x, act=F.relu)

    def hgblock(self, li, c1, cm, c2, k, light, shortcut, x):
        y = [x]
        for i in range(6):
            y.append(self.lightconv(f"model.{li}.m.{i}", y[-1], k) if light else self.conv(f"model.{li}.m.{i}", y[-1], act=F.relu))
        y = self.conv(f"model.{li}.ec", self.conv(f"model.{li}.sc", torch.cat(y, 1), act=F.relu), act=F.relu)
        return y + x if shortcut and c1 == c2 else y

    def repc3(self, li, x):
        a = self.conv(f"model.{li}.cv1", x, act=F.silu)
        for j in range(3):
            a = self.repconv(f"model.{li}.m.{j}", a)
        return a + self.conv(f"model.{li}.cv2", x, act=F.silu)

    # ---- nn/modules/transformer.py ----
    def linear(self, p, x):
        return F.linear(x, self.t(p + ".weight"), self.t(p + ".bias"))

    def layer_norm(self, p, x):
        return F.layer_norm(x, (x.shape[-1],), self.t(p + ".weight"), self.t(p + ".bias"), 1e-5)

    def mha(self, p, q, k, v):
        """nn.MultiheadAttention(batch_first=False) on [B, L, C] inputs (the caller's transposes undone), eval, no mask."""
        if p + ".in_proj_weight" in self.sd:
            w, b = self.t(p + ".in_proj_weight").chunk(3), self.t(p + ".in_proj_bias").chunk(3)
        else:
            w = [self.t(f"{p}.{n}_proj.weight") for n in "qkv"]
            b = [self.t(f"{p}.{n}_proj.bias") for n in "qkv"]
        B, L, C = q.shape
        hd = C // NH
        qh = F.linear(q, w[0], b[0]).view(B, L, NH, hd).transpose(1, 2)
        kh = F.linear(k, w[1], b[1]).view(B, k.shape[1], NH, hd).transpose(1, 2)
        vh = F.linear(v, w[2], b[2]).view(B, v.shape[1], NH, hd).transpose(1, 2)
        a = torch.softmax((qh / math.sqrt(hd)) @ kh.transpose(-1, -2), -1)
        o = (a @ vh).transpose(1, 2).reshape(B, L, C)
        return self.linear(p + ".out_proj", o)

    def aifi(self, x):
        c, h, w = x.shape[1:]
        pos = pos_embed(w, h, c, self.dt)
        src = x.flatten(2).permute(0, 2, 1)
        q = src + pos
        src = self.layer_norm("model.11.norm1", src + self.mha("model.11.ma", q, q, src))
        src2 = self.linear("model.11.fc2", F.gelu(self.linear("model.11.fc1", src)))
        src = self.layer_norm("model.11.norm2", src + src2)
        return src.permute(0, 2, 1).reshape(-1, c, h, w)

    def mlp(self, p, x, n=3):
        for i in range(n):
            x = self.linear(f"{p}.layers.{i}", x)
            if i < n - 1:
                x = F.relu(x)
        return x

    def ms_deform_attn(self, p, query, refer_bbox, value, shapes):
        bs, len_q = query.shape[:2]
        len_v = value.shape[1]
        value = self.linear(p + ".value_proj", value).view(bs, len_v, NH, HD // NH)
        off = self.linear(p + ".sampling_offsets", query).view(bs, len_q, NH, NL, NP, 2)
        aw = torch.softmax(self.linear(p + ".attention_weights", query).view(bs, len_q, NH, NL * NP), -1).view(bs, len_q, NH, NL, NP)
        ref = refer_bbox[:, :, None, :]
        loc = ref[:, :, None, :, None, :2] + off / NP * ref[:, :, None, :, None, 2:] * 0.5
        out = multi_scale_deformable_attn(value, shapes, loc, aw)
        return self.linear(p + ".output_proj", out)

    def decoder_layer(self, i, embed, refer_bbox, feats, shapes, query_pos):
        p = f"model.28.decoder.layers.{i}"
        q = embed + query_pos
        embed = self.layer_norm(p + ".norm1", embed + self.mha(p + ".self_attn", q, q, embed))
        tgt = self.ms_deform_attn(p + ".cross_attn", embed + query_pos, refer_bbox, feats, shapes)
        embed = self.layer_norm(p + ".norm2", embed + tgt)
        tgt2 = self.linear(p + ".linear2", F.relu(self.linear(p + ".linear1", embed)))
        return self.layer_norm(p + ".norm3", embed + tgt2)

    # ---- the whole model ----
    def forward(self, x: torch.Tensor) -> dict:
        """x: [B, 3, H, W] RGB in [0, 1] -> {"boxes": [B,300,4] cxcywh, "scores": [B,300,nc] after the sigmoid, "topk": [B,300] token
        indices, "enc_max": [B, tokens] max encoder logit per token}."""
        x = x.to(self.dt)
        y = {}
        x = self.hgstem(x)
        blocks = {b[0]: b for b in HGBLOCKS}
        for li in range(1, 10):
            if li in blocks:
                x = self.hgblock(*blocks[li], x)
            else:
                x = self.conv(f"model.{li}", x, 2, g=x.shape[1])
            y[li] = x
        x = self.conv("model.10", y[9])
        x = self.aifi(x)
        y[12] = x = self.conv("model.12", x, act=F.silu)
        x = torch.cat([F.interpolate(x, scale_factor=2, mode="nearest"), self.conv("model.14", y[7])], 1)
        x = self.repc3(16, x)
        y[17] = x = self.conv("model.17", x, act=F.silu)
        x = torch.cat([F.interpolate(x, scale_factor=2, mode="nearest"), self.conv("model.19", y[3])], 1)
        y[21] = x = self.repc3(21, x)
        x = torch.cat([self.conv("model.22", x, 2, act=F.silu), y[17]], 1)
        y[24] = x = self.repc3(24, x)
        x = torch.cat([self.conv("model.25", x, 2, act=F.silu), y[12]], 1)
        y[27] = self.repc3(27, x)
        return self.decoder([y[21], y[24], y[27]])

    def decoder(self, xs):
        d = "model.28"
        feats, shapes = [], []
        for i, f in enumerate(xs):
            w = self.t(f"{d}.input_proj.{i}.0.weight")
            if f"{d}.input_proj.{i}.1.weight" in self.sd:
                f = F.conv2d(f, w)
                f = F.batch_norm(f, self.t(f"{d}.input_proj.{i}.1.running_mean"), self.t(f"{d}.input_proj.{i}.1.running_var"),
                                 self.t(f"{d}.input_proj.{i}.1.weight"), self.t(f"{d}.input_proj.{i}.1.bias"), False, 0.0, BN_EPS)
            else:
                f = F.conv2d(f, w, self.t(f"{d}.input_proj.{i}.0.bias"))
            shapes.append(list(f.shape[2:]))
            feats.append(f.flatten(2).permute(0, 2, 1))
        feats = torch.cat(feats, 1)
        bs = feats.shape[0]
        anchors, valid = generate_anchors(shapes, self.dt)
        feat = self.layer_norm(f"{d}.enc_output.1", self.linear(f"{d}.enc_output.0", valid * feats))
        scores = self.linear(f"{d}.enc_score_head", feat)
        enc_max = scores.max(-1).values
        topk = topk_lowest_index(enc_max, NQ)
        bi = torch.arange(bs).unsqueeze(-1).repeat(1, NQ).view(-1)
        tf = feat[bi, topk.view(-1)].view(bs, NQ, -1)
        ta = anchors[:, topk.view(-1)].view(bs, NQ, -1)
        refer = self.mlp(f"{d}.enc_bbox_head", tf) + ta
        embed = tf
        refer = refer.sigmoid()
        for i in range(6):
            pos = self.mlp(f"{d}.query_pos_head", refer, 2)
            embed = self.decoder_layer(i, embed, refer, feats, shapes, pos)
            refer = torch.sigmoid(self.mlp(f"{d}.dec_bbox_head.{i}", embed) + inverse_sigmoid(refer))
        sc = torch.sigmoid(self.linear(f"{d}.dec_score_head.5", embed))
        return {"boxes": refer, "scores": sc, "topk": topk, "enc_max": enc_max}


# ---- functions ----------------------------------------------------------------------------------------------------------------------
def pos_embed(w, h, embed_dim=256, dtype=torch.float64, temperature=10000.0):
    """AIFI.build_2d_sincos_position_embedding (float32 arithmetic, as the library), in `dtype`: [1, w*h, embed_dim]."""
    grid_w = torch.arange(w, dtype=torch.float32)
    grid_h = torch.arange(h, dtype=torch.float32)
    grid_w, grid_h = torch.meshgrid(grid_w, grid_h, indexing="ij")
    pos_dim = embed_dim // 4
    omega = torch.arange(pos_dim, dtype=torch.float32) / pos_dim
    omega = 1.0 / (temperature ** omega)
    out_w = grid_w.flatten()[..., None] @ omega[None]
    out_h = grid_h.flatten()[..., None] @ omega[None]
    return torch.cat([torch.sin(out_w), torch.cos(out_w), torch.sin(out_h), torch.cos(out_h)], 1)[None].to(dtype)


def generate_anchors(shapes, dtype=torch.float64, grid_size=0.05, eps=1e-2):
    """RTDETRDecoder._generate_anchors: ([1, tokens, 4] logit anchors with inf where invalid, [1, tokens, 1] valid mask)."""
    anchors = []
    for i, (h, w) in enumerate(shapes):
        sy = torch.arange(end=h, dtype=dtype)
        sx = torch.arange(end=w, dtype=dtype)
        grid_y, grid_x = torch.meshgrid(sy, sx, indexing="ij")
        grid_xy = torch.stack([grid_x, grid_y], -1)
        valid_wh = torch.tensor([w, h], dtype=dtype)
        grid_xy = (grid_xy.unsqueeze(0) + 0.5) / valid_wh
        wh = torch.ones_like(grid_xy, dtype=dtype) * grid_size * (2.0 ** i)
        anchors.append(torch.cat([grid_xy, wh], -1).view(-1, h * w, 4))
    anchors = torch.cat(anchors, 1)
    valid = ((anchors > eps) & (anchors < 1 - eps)).all(-1, keepdim=True)
    anchors = torch.log(anchors / (1 - anchors))
    anchors = anchors.masked_fill(~valid, float("inf"))
    return anchors, valid


def topk_lowest_index(s: torch.Tensor, k: int) -> torch.Tensor:
    """torch.topk(s, k, dim=1).indices with a defined order for ties (descending score, then ascending index), as the device's
    radix select. torch.topk itself promises no order among equal values."""
    out = []
    for row in s:
        idx = np.lexsort((np.arange(row.numel()), -row.numpy()))
        out.append(torch.from_numpy(idx[:k].copy()))
    return torch.stack(out)


def inverse_sigmoid(x, eps=1e-5):
    x = x.clamp(min=0, max=1)
    x1 = x.clamp(min=eps)
    x2 = (1 - x).clamp(min=eps)
    return torch.log(x1 / x2)


def multi_scale_deformable_attn(value, shapes, loc, aw):
    """multi_scale_deformable_attn_pytorch (F.grid_sample bilinear, zeros padding, align_corners=False)."""
    bs, _, nh, ed = value.shape
    _, nq, nh, nl, npt, _ = loc.shape
    value_list = value.split([h * w for h, w in shapes], dim=1)
    grids = 2 * loc - 1
    vals = []
    for lv, (h, w) in enumerate(shapes):
        v = value_list[lv].flatten(2).transpose(1, 2).reshape(bs * nh, ed, h, w)
        g = grids[:, :, :, lv].transpose(1, 2).flatten(0, 1)
        vals.append(F.grid_sample(v, g, mode="bilinear", padding_mode="zeros", align_corners=False))
    aw = aw.transpose(1, 2).reshape(bs * nh, 1, nq, nl * npt)
    out = (torch.stack(vals, dim=-2).flatten(-2) * aw).sum(-1).view(bs, nh * ed, nq)
    return out.transpose(1, 2).contiguous()


# ---- RTDETRPredictor ---------------------------------------------------------------------------------------------------------------
def preprocess(img_bgr: np.ndarray, imgsz: int = 640) -> torch.Tensor:
    """LetterBox(imgsz, auto=False, scale_fill=True) (cv2 INTER_LINEAR stretch, no padding), BGR -> RGB, / 255: [1, 3, imgsz, imgsz]."""
    im = resize_linear_u8(img_bgr, imgsz, imgsz)
    return torch.from_numpy(np.ascontiguousarray(im[..., ::-1].transpose(2, 0, 1)).astype(np.float32) / 255.0)[None]


def postprocess(boxes: np.ndarray, scores: np.ndarray, orig_shape, conf: float = 0.25) -> np.ndarray:
    """RTDETRPredictor.postprocess for one image: [n, 6] (x1, y1, x2, y2, score, cls) in original pixels, query order, no NMS."""
    b = torch.as_tensor(boxes)
    s = torch.as_tensor(scores)
    xy = torch.empty_like(b)
    dw, dh = b[..., 2] / 2, b[..., 3] / 2
    xy[..., 0] = b[..., 0] - dw
    xy[..., 1] = b[..., 1] - dh
    xy[..., 2] = b[..., 0] + dw
    xy[..., 3] = b[..., 1] + dh
    ms, cls = s.max(-1, keepdim=True)
    idx = ms.squeeze(-1) > conf
    pred = torch.cat([xy, ms, cls.to(xy.dtype)], -1)[idx]
    oh, ow = orig_shape[:2]
    pred[..., [0, 2]] *= ow
    pred[..., [1, 3]] *= oh
    return pred.numpy()


def predict(ref: Ref, img_bgr: np.ndarray, imgsz: int = 640, conf: float = 0.25) -> np.ndarray:
    with torch.no_grad():
        o = ref.forward(preprocess(img_bgr, imgsz))
    return postprocess(o["boxes"][0].float().numpy(), o["scores"][0].float().numpy(), img_bgr.shape, conf)
