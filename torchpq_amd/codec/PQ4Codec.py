"""Product quantiser, 4 bits per sub-vector: 16 centroids per sub-quantizer, two sub-quantizers per code byte
(include/torchpq_amd.h: byte b holds sub-quantizer 2 b in bits 0-3 and sub-quantizer 2 b + 1 in bits 4-7)."""
import torch

from ..clustering import MultiKMeans
from .BaseCodec import BaseCodec


class PQ4Codec(BaseCodec):
    n_clusters = 16

    def __init__(self, d_vector, n_subvectors=8, distance="euclidean", verbose=0):
        super().__init__()
        assert d_vector % n_subvectors == 0
        assert n_subvectors % 2 == 0, "two sub-quantizers share a code byte"
        self.n_subvectors = n_subvectors
        self.d_vector = d_vector
        self.d_subvector = d_vector // n_subvectors
        self.distance = distance
        self.verbose = verbose
        self.kmeans = MultiKMeans(n_clusters=self.n_clusters, distance=distance, max_iter=25, verbose=verbose)

    @property
    def codebook(self):
        """[n_subvectors, d_subvector, 16] or None before training"""
        return self.kmeans.centroids if self.is_trained else None

    @staticmethod
    def pack_nibbles(labels):
        """labels [m, n] (integers 0 ... 15, m even) -> packed [m // 2, n] uint8"""
        assert labels.dim() == 2 and labels.shape[0] % 2 == 0
        labels = labels.to(torch.uint8)
        return labels[0::2] | (labels[1::2] << 4)

    @staticmethod
    def unpack_nibbles(packed):
        """packed [m // 2, n] uint8 -> labels [m, n] uint8 (the inverse of pack_nibbles)"""
        assert packed.dim() == 2 and packed.dtype == torch.uint8
        return torch.stack((packed & 15, packed >> 4), dim=1).reshape(2 * packed.shape[0], packed.shape[1])

    def train(self, x):
        """x [d_vector, n_data] f32"""
        d_vector, n_data = x.shape
        assert d_vector == self.d_vector
        y = self.kmeans.fit(x.reshape(self.n_subvectors, self.d_subvector, n_data))
        self._trained(True)
        return y

    def encode(self, x):
        """x [d_vector, n_data] f32 -> packed codes [n_subvectors // 2, n_data] uint8"""
        assert self.is_trained, "codec is not trained"
        d_vector, n_data = x.shape
        assert d_vector == self.d_vector
        x = x.reshape(self.n_subvectors, self.d_subvector, n_data)
        _, labels = self.kmeans.get_labels(x, self.codebook)
        return self.pack_nibbles(labels)

    def decode(self, code):
        """packed codes [n_subvectors // 2, n_data] uint8 -> [d_vector, n_data] f32"""
        assert self.is_trained, "codec is not trained"
        assert code.shape[0] * 2 == self.n_subvectors
        labels = self.unpack_nibbles(code.to(self.codebook.device)).long()
        index = labels[:, None, :].expand(self.n_subvectors, self.d_subvector, labels.shape[1])
        return torch.gather(self.codebook, 2, index).reshape(self.d_vector, labels.shape[1])
