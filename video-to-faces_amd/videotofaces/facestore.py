"""The decoded faces of a full run, kept in HBM between the detection and the grouping stage
(video_to_faces(face_handoff='device')).

The detection stage's device encoder leaves, next to every face file it writes, the pixels that
file decodes to (utils.jpeg_encode_crops(decoded=True)): one tensor per det-batch, a "chunk".
The store maps a face file's path to its place in its chunk; encode_faces then gathers the stored
faces into its atlas (utils.faces_to_atlas) instead of reading and decoding the files.  The
bookkeeping touches no GPU API: a chunk is any uint8 tensor.

HANDOFF_BYTES is the budget of one store: 16 GiB, about 5 % of an MI355X's 288 GB of HBM, which
leaves the models, their scratch arenas and the grouping stage's atlases (1 GiB each) ample room.
A face of 160 x 160 pixels takes 75 KiB, so the budget holds about 220,000 of them; a det-batch
that would take the store past it is not stored, and its faces travel by file as they do without
a store.
"""

HANDOFF_BYTES = 16 << 30


class FaceStore:
    def __init__(self, budget=None):
        self.budget = HANDOFF_BYTES if budget is None else int(budget)
        self.nbytes = 0    # bytes of the chunks held
        self._faces = {}   # name -> (chunk id, byte offset, h, w)
        self._chunks = {}  # chunk id -> [tensor, faces still stored]
        self._next = 0

    def __len__(self):
        return len(self._faces)

    def __contains__(self, name):
        return name in self._faces

    def add(self, names, pixels, offsets, sizes, keep=None):
        """One encode call's faces: `pixels` its uint8 1-D tensor, face i (named names[i], sizes[i] =
        (h, w)) at pixels[offsets[i]:offsets[i] + h * w * 3]; keep: a mask, faces with a false entry
        are not stored (their bytes stay part of the chunk).  A name that is stored already is
        replaced.  -> False, with the store unchanged, when the chunk would take it past the budget."""
        import torch
        if not (isinstance(pixels, torch.Tensor) and pixels.dtype == torch.uint8 and pixels.dim() == 1):
            raise ValueError('pixels must be a uint8 1-D tensor')
        names = list(names)
        if not (len(offsets) >= len(names) and len(sizes) == len(names) and (keep is None or len(keep) == len(names))):
            raise ValueError('names, offsets, sizes and keep must describe the same faces')
        entries = []
        for i, name in enumerate(names):
            h, w, at = int(sizes[i][0]), int(sizes[i][1]), int(offsets[i])
            if h < 0 or w < 0 or at < 0 or at + h * w * 3 > pixels.numel():
                raise ValueError('face %d lies outside pixels' % i)
            if keep is None or keep[i]:
                entries.append((name, at, h, w))
        if not entries:
            return True
        if self.nbytes + pixels.numel() > self.budget:
            return False
        self.drop([name for name, _, _, _ in entries])
        cid, self._next = self._next, self._next + 1
        self._chunks[cid] = [pixels, 0]
        self.nbytes += pixels.numel()
        for name, at, h, w in entries:
            if name in self._faces:  # twice in this call: the later one stays
                self._chunks[cid][1] -= 1
            self._faces[name] = (cid, at, h, w)
            self._chunks[cid][1] += 1
        return True

    def get(self, name):
        """-> (chunk tensor, byte offset, h, w), or None for a name that is not stored"""
        e = self._faces.get(name)
        if e is None:
            return None
        return self._chunks[e[0]][0], e[1], e[2], e[3]

    def drop(self, names):
        """Forget these faces (unknown names are ignored); a chunk is released with its last face."""
        for name in names:
            e = self._faces.pop(name, None)
            if e is None:
                continue
            chunk = self._chunks[e[0]]
            chunk[1] -= 1
            if chunk[1] == 0:
                self.nbytes -= chunk[0].numel()
                del self._chunks[e[0]]

    def clear(self):
        self._faces.clear()
        self._chunks.clear()
        self.nbytes = 0
