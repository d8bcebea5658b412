"""PdsNetwork: the dependency-injected pipeline that consumes the hot-path modules.

Same constructor, ``set_maximum_disparity``, ``pass_through_network``, ``forward`` and
``default`` as reference practical_deep_stereo/network.py:14-65, so a ``PdsTrainer``-style loop
can use it unchanged; ``default()`` wires the MI355X modules of this package instead of the
reference classes.  In eval mode, when the injected modules are this package's Regularization and
SubpixelMap, the last regularization layer and the estimator run fused.
"""
import collections

import torch
from torch import nn

from practicaldeepstereo_nips2018_amd import consistency
from practicaldeepstereo_nips2018_amd import embedding
from practicaldeepstereo_nips2018_amd import estimator
from practicaldeepstereo_nips2018_amd import matching
from practicaldeepstereo_nips2018_amd import regularization
from practicaldeepstereo_nips2018_amd import size_adapter


# PdsNetwork.forward_left_right: both views [batch, H, W] (filled with fill=True) and their masks (torch.bool)
LeftRightDisparity = collections.namedtuple('LeftRightDisparity', ['left', 'right', 'left_valid', 'right_valid'])

# forward_left_right's second stream, one per device (shared by every network: stream order keeps calls apart)
_right_view_streams = {}


def _right_view_stream(device):
    index = device.index if device.index is not None else torch.cuda.current_device()
    if index not in _right_view_streams:
        _right_view_streams[index] = torch.cuda.Stream(torch.device('cuda', index))
    return _right_view_streams[index]


class PdsNetwork(nn.Module):
    def __init__(self, size_adapter_module, embedding_module, matching_module,
                 regularization_module, estimator_module):
        super(PdsNetwork, self).__init__()
        self._size_adapter = size_adapter_module
        self._embedding = embedding_module
        self._matching = matching_module
        self._regularization = regularization_module
        self._estimator = estimator_module
        self.fuse_estimator = True

    def set_maximum_disparity(self, maximum_disparity):
        if (maximum_disparity + 1) % 64 != 0:
            raise ValueError(
                '"maximum_disparity" + 1 should be multiple of 64, e.g.,'
                '"maximum disparity" can be equal to 63, 191, 255, 319...')
        self._maximum_disparity = maximum_disparity
        # the embedding downsamples 4x, so Matching covers (max + 1) / 4 planes (network.py:33-36)
        self._matching.set_maximum_disparity((maximum_disparity + 1) // 4 - 1)

    def freeze_weights(self):
        """Inference deployment: promise that the parameters stay untouched, so the modules keep their re-laid-out
        weights between calls (``_lib.FrozenWeightsMixin``; not in the reference).  ``train()`` undoes it;
        ``.to()`` and ``load_state_dict`` invalidate the kept weights once (the network stays frozen); after editing
        parameters through ``.data`` call ``invalidate_weights()`` yourself."""
        for module in self.modules():
            if module is not self and hasattr(module, 'freeze_weights'):
                module.freeze_weights()
        return self

    def invalidate_weights(self):
        for module in self.modules():
            if module is not self and hasattr(module, 'invalidate_weights'):
                module.invalidate_weights()
        return self

    def _signatures(self, left_image, right_image):
        left_descriptor, shortcut_from_left = self._embedding(left_image)
        right_descriptor = self._embedding(right_image)[0]
        return self._matching(left_descriptor, right_descriptor), shortcut_from_left

    def _can_fuse_padding(self, left_image, right_image):
        return (isinstance(self._embedding, embedding.Embedding)
                and isinstance(self._size_adapter, size_adapter.SizeAdapter)
                and left_image.shape == right_image.shape and left_image.is_cuda)

    def _signatures_from_unpadded(self, left_image, right_image, mirror=False):
        """Both images through ONE embedding call (InstanceNorm statistics are per image, so batching them is
        the same arithmetic as network.py:38-40) with SizeAdapter.pad applied inside its loader.  ``mirror``: the
        signatures of the mirrored pair, flip(left_image) and flip(right_image), read mirrored by that loader."""
        pad_top, pad_left = self._size_adapter.measure(left_image)
        batch = left_image.size(0)
        descriptors, shortcuts = self._embedding.forward_padded(
            torch.cat([left_image, right_image], 0), pad_top, pad_left, mirror=mirror)
        return self._matching(descriptors[:batch], descriptors[batch:]), shortcuts[:batch]

    def pass_through_network(self, left_image, right_image):
        signatures, shortcut_from_left = self._signatures(left_image, right_image)
        return self._regularization(signatures, shortcut_from_left), shortcut_from_left

    def _can_fuse(self):
        return (self.fuse_estimator and isinstance(self._regularization, regularization.Regularization)
                and isinstance(self._estimator, estimator.SubpixelMap))

    def forward(self, left_image, right_image):
        """Sub-pixel disparity in eval mode, matching cost in training mode (network.py:45-52)."""
        if self._can_fuse_padding(left_image, right_image):
            signatures, shortcut_from_left = self._signatures_from_unpadded(left_image, right_image)
        else:
            signatures, shortcut_from_left = self._signatures(self._size_adapter.pad(left_image),
                                                              self._size_adapter.pad(right_image))
        if not self.training and self._can_fuse():
            crop = self._size_adapter.padding() if hasattr(self._size_adapter, 'padding') else None
            if crop is not None and self._regularization.can_fold_crop(self._estimator):
                # SizeAdapter.unpad (size_adapter.py:45-52) folded into the estimator's store: the result is the
                # contiguous [batch, H, W] image, not a view of the padded one
                return self._regularization.forward_with_estimator(signatures, shortcut_from_left, self._estimator,
                                                                   crop=crop)
            output = self._regularization.forward_with_estimator(signatures, shortcut_from_left,
                                                                 self._estimator)
        else:
            output = self._regularization(signatures, shortcut_from_left)
            if not self.training:
                output = self._estimator(output)
        return self._size_adapter.unpad(output)

    def forward_with_confidence(self, left_image, right_image):
        """Eval mode only (not in the reference): -> (disparity, confidence), both [batch, H, W].  The disparity is the
        one ``forward`` returns; the confidence is the estimator's window share of the softmax over all planes
        (``SubpixelMap.with_confidence``), from the same sweep.  Same padding fusion, estimator fusion and crop folding
        as ``forward``, and the same unfused fall-back."""
        if self.training:
            raise RuntimeError('forward_with_confidence is inference only: call eval() first (in training mode the '
                               'network returns the matching cost, network.py:45-52)')
        if self._can_fuse_padding(left_image, right_image):
            signatures, shortcut_from_left = self._signatures_from_unpadded(left_image, right_image)
        else:
            signatures, shortcut_from_left = self._signatures(self._size_adapter.pad(left_image),
                                                              self._size_adapter.pad(right_image))
        if self._can_fuse():
            crop = self._size_adapter.padding() if hasattr(self._size_adapter, 'padding') else None
            if crop is not None and self._regularization.can_fold_crop(self._estimator):
                return self._regularization.forward_with_estimator(signatures, shortcut_from_left, self._estimator,
                                                                   crop=crop, with_confidence=True)
            disparity, confidence = self._regularization.forward_with_estimator(
                signatures, shortcut_from_left, self._estimator, with_confidence=True)
        else:
            if not hasattr(self._estimator, 'with_confidence'):
                raise TypeError('forward_with_confidence needs an estimator with a with_confidence method '
                                '(SubpixelMap), got %s' % type(self._estimator).__name__)
            disparity, confidence = self._estimator.with_confidence(
                self._regularization(signatures, shortcut_from_left))
        return self._size_adapter.unpad(disparity), self._size_adapter.unpad(confidence)

    def forward_right(self, left_image, right_image, with_confidence=False):
        """Eval mode only (not in the reference): the disparity of the RIGHT view, [batch, H, W],

            D_R(L, R) = flip(forward(flip(R), flip(L)))        flip = torch.flip(., [-1])

        bit for bit (with ``with_confidence``: (disparity, confidence) of ``forward_with_confidence``, mirrored alike).
        The network only learned left-reference geometry (the match lies to the left, S_d(R)[x] = R[x - d]); mirroring
        both images and swapping them gives the right view that geometry.  The mirrors are folded into the kernels: one
        embedding call over cat([R, L]) reads both images mirrored, and the fused regularization + estimator tail
        stores its cropped columns mirrored.  Same padding fusion, estimator fusion and unfused fall-back as
        ``forward`` (where a kernel cannot fold the mirror, the result is flipped).  Runs without autograd."""
        if self.training:
            raise RuntimeError('forward_right is inference only: call eval() first (in training mode the network '
                               'returns the matching cost, network.py:45-52)')
        with torch.no_grad():
            if self._can_fuse_padding(left_image, right_image):
                signatures, shortcut_from_left = self._signatures_from_unpadded(right_image, left_image, mirror=True)
            else:
                signatures, shortcut_from_left = self._signatures(
                    self._size_adapter.pad(torch.flip(right_image, [-1])),
                    self._size_adapter.pad(torch.flip(left_image, [-1])))
            if self._can_fuse():
                crop = self._size_adapter.padding() if hasattr(self._size_adapter, 'padding') else None
                if crop is not None and self._regularization.can_fold_crop(self._estimator):
                    # the crop and the mirror both folded into the store
                    return self._regularization.forward_with_estimator(
                        signatures, shortcut_from_left, self._estimator, crop=crop, with_confidence=with_confidence,
                        mirror=True)
                output = self._regularization.forward_with_estimator(signatures, shortcut_from_left, self._estimator,
                                                                     with_confidence=with_confidence)
            else:
                cost = self._regularization(signatures, shortcut_from_left)
                if with_confidence:
                    if not hasattr(self._estimator, 'with_confidence'):
                        raise TypeError('forward_right(with_confidence=True) needs an estimator with a '
                                        'with_confidence method (SubpixelMap), got %s' %
                                        type(self._estimator).__name__)
                    output = self._estimator.with_confidence(cost)
                else:
                    output = self._estimator(cost)
            if with_confidence:
                return tuple(torch.flip(self._size_adapter.unpad(o), [-1]) for o in output)
            return torch.flip(self._size_adapter.unpad(output), [-1])

    def forward_left_right(self, left_image, right_image, max_difference=1.0, fill=False):
        """Eval mode only (not in the reference): both views' disparities and the left-right consistency check,
        -> ``LeftRightDisparity(left, right, left_valid, right_valid)``, all [batch, H, W].

        ``left`` is computed as ``forward`` computes it and ``right`` as ``forward_right`` does, as two batch-B passes
        (batching the two views would not be bit-equal): the right view runs on a second stream,
        beside the left one, and the caller's stream waits for it.  Then ``consistency.left_right_check`` runs on the
        caller's stream; with ``fill=True`` ``left`` / ``right`` are the filled maps (invalid pixels take the minimum of
        their nearest valid neighbours on the row), and the masks still say which pixels passed.  Runs without
        autograd."""
        if self.training:
            raise RuntimeError('forward_left_right is inference only: call eval() first (in training mode the network '
                               'returns the matching cost, network.py:45-52)')
        consistency._check_max_difference(max_difference)
        with torch.no_grad():
            if isinstance(left_image, torch.Tensor) and left_image.is_cuda:
                device = left_image.device
                caller = torch.cuda.current_stream(device)
                side = _right_view_stream(device)
                side.wait_stream(caller)   # the images were produced on the caller's stream
                with torch.cuda.stream(side):
                    right = self.forward_right(left_image, right_image)
                left = self.forward(left_image, right_image)
                caller.wait_stream(side)
                # memory used across the two streams: not reused before the other stream is done with it
                for t in (left_image, right_image):
                    if isinstance(t, torch.Tensor) and t.is_cuda:
                        t.record_stream(side)
                right.record_stream(caller)
            else:
                right = self.forward_right(left_image, right_image)   # (raises: no CPU fallback)
                left = self.forward(left_image, right_image)
            checked = consistency.left_right_check(left, right, max_difference, fill=fill)
        if fill:
            return LeftRightDisparity(*checked)
        return LeftRightDisparity(left, right, *checked)

    @staticmethod
    def default(maximum_disparity=255):
        network = PdsNetwork(
            size_adapter_module=size_adapter.SizeAdapter(),
            embedding_module=embedding.Embedding(),
            matching_module=matching.Matching(operation=matching.MatchingOperation(),
                                              maximum_disparity=0),
            regularization_module=regularization.Regularization(),
            estimator_module=estimator.SubpixelMap())
        network.set_maximum_disparity(maximum_disparity)
        return network
