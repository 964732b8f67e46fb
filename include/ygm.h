/*
 * ygm.h -- C ABI of the MI355X batched Yjs update engine ("ygm" = Yjs GPU Merge).
 *
 * The drop-in boundary for Hocuspocus's persistence / sync hot path.  Plain
 * pointers and sizes only (no torch, no HIP types in signatures).  Each entry
 * point replaces a per-document yjs call that the reference makes one document
 * at a time on the Node event loop:
 *
 *   ygm_merge_v1           <- Y.mergeUpdates(updates)                  (yjs Y@37704; the
 *                             store path packages/extension-database/src/Database.ts:55-60
 *                             persists Y.encodeStateAsUpdate(doc); the GPU extension persists
 *                             mergeUpdates([snapshot, ...onChange updates]) instead,
 *                             packages/server/src/Hocuspocus.ts:244-277,417-447)
 *   ygm_diff_v1            <- Y.diffUpdate(update, stateVector)        (yjs Y@41210; the Step1 ->
 *                             Step2 reply of packages/server/src/MessageReceiver.ts:137-155)
 *   ygm_sv_from_update_v1  <- Y.encodeStateVectorFromUpdate(update)    (yjs Y@38304; the SV a
 *                             server sends in SyncStep1, packages/server/src/OutgoingMessage.ts:93-99)
 *
 * Byte-for-byte identical to yjs 13.6.26 by default; YGM_F_COMPAT_135 selects
 * the yjs 13.5.16 / lib0 0.2.42 behaviours.  A document whose
 * content yjs would re-encode (non-canonical Any/JSON) is
 * refused with YGM_ENONCANON instead of being silently copied.
 *
 * Error behaviour mirrors the reference: yjs throws per document; here the
 * batch call succeeds and the failing document carries a non-zero status
 * (the extension then rejects only that document's hook, Hocuspocus.ts:431-435).
 */
#ifndef YGM_H
#define YGM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- per-document status codes ------------------------------------------ */
#define YGM_OK 0
#define YGM_EMALFORMED 1   /* yjs throws: truncated input, bad UTF-8, unknown content/Any tag, bad JSON */
#define YGM_ERANGE 2       /* yjs throws "Integer out of Range": varuint > 2^53 */
#define YGM_ENONCANON 3    /* yjs would re-encode content (non-canonical Any/JSON): refused, not copied */
#define YGM_ESURROGATE 4   /* compat 13.5 only: lib0 0.2.42 throws writing a lone surrogate */
#define YGM_EDEPTH 5       /* Any/JSON nesting deeper than YGM_MAX_DEPTH */
#define YGM_ENOMEM 6
#define YGM_EDEVICE 7      /* HIP error / device fault */
#define YGM_EINVAL 8       /* bad call arguments */
#define YGM_EUNSUPPORTED 9 /* snapshot / step2 / contains only: the update repeats a client block or overlaps
                              structs (yjs's writers never do), or names a non-type item as a parent
                              -- the caller keeps its yjs path for that document */

#define YGM_MAX_DEPTH 32

/* ---- context flags -------------------------------------------------------- */
#define YGM_F_COMPAT_135 1u   /* delete-set clients in first-seen order; lone surrogate -> error */
#define YGM_F_FORCE_SEQ 2u    /* route every merge through the exact sequential kernel (testing) */
#define YGM_F_KEEP_SUB 4u     /* internal to ygm_sync_step2_v1: diffs keep each struct's parentSub bit (0x20) */
#define YGM_F_FLOATS 8u       /* opt-in, given to ygm_open: ygm_json_v1, ygm_json_fields_v1, ygm_tojson_v1 (their _device
                                 forms and the version forms built on them) write the numbers they refuse without it -- a
                                 finite float32 / float64 of a ContentAny as Number.prototype.toString writes it (the
                                 shortest decimal that reads back as the same double, JavaScript's layout: 103.5, 1e+21,
                                 1.5e-7; an integer above 2^53 likewise, 2^60 is 1152921504606847000; a float32 widened
                                 exactly first, 0.1f is 0.10000000149011612), and non-integer numbers inside ContentJSON,
                                 format and embed values as the canonical text they already are.  Still refused with the
                                 flag: JSON text holding a number of more than 15 significant digits or with an exponent
                                 (the state's parse calls it not canonical: YGM_ENONCANON), BigInt, Uint8Array, the
                                 undefined rules, __proto__, hashed mark names.  Without the flag every call returns what
                                 it returned before the flag existed; every other entry point ignores it
                                 (ygm_convert_v2_to_v1 keeps its refusal). */
#define YGM_F_SNAP_STATE 16u  /* internal to ygm_contains_v1: such a state's snapshot is its integrated part alone
                                 (Y.snapshot(doc): the store's state vector and delete set) */
#define YGM_F_SNAP_NOGC 32u   /* internal to ygm_version_restore_v1: every document of the batch is snapshotted as a
                                 Y.Doc({gc: false}) (what YGM_DOC_NO_GC sets per document) */
#define YGM_F_SNAP_VERSION 64u /* internal to ygm_version_take_v1: the snapshot batch ends with the encoded Snapshot V1 */

typedef struct ygm_ctx ygm_ctx;

/* Result of one host-API batch call.  Owned by the context (pinned host
 * memory); valid until the next call on the same context or ygm_close.
 * Document d's output is data[off[d] .. off[d]+len[d]) when status[d] ==
 * YGM_OK (len[d] = 0 otherwise); outputs are packed in document order.
 * The host API moves a batch in chunks of whole documents through two
 * stage streams (pinned staging, H2D of chunk i+1 beside the kernels of
 * chunk i, device-side packing, D2H of the packed outputs only); h2d_ms /
 * d2h_ms in ygm_stats_t are those copies' event times. */
typedef struct {
  const uint8_t *data;
  const uint64_t *off;
  const uint64_t *len;
  const int32_t *status;
  uint32_t n_docs;
  uint64_t data_bytes;
} ygm_result;

typedef struct {
  uint64_t calls, docs, updates;
  uint64_t bytes_in, bytes_out;       /* algorithmic bytes */
  uint64_t docs_fast, docs_seq;        /* documents finished by the general tiers (merge: wave / workgroup kernels;
                                          SV / diff: the exact per-document kernel) / by the sequential merge kernel */
  double kernel_ms, h2d_ms, d2h_ms;    /* cumulative, HIP-event timed */
  uint64_t docs_lean;                  /* documents finished by the lean kernels (merge: the debounce-log kernels; SV / diff:
                                          lane-per-document walker) */
  double lean_ms;                      /* HIP-event time of the lean kernel launches (part of kernel_ms): one span
                                          from the first launch after a finish to that finish */
  uint64_t lean_launches;              /* lean kernel launches timed in lean_ms */
  uint64_t docs_big;                   /* merges finished by the large-document ([snapshot, ...log]) kernel */
  uint64_t docs_lean_wide;             /* merges of docs_lean finished by the wide lean kernel (updates <= 64 B,
                                          documents <= 7 KB: the narrow kernel's deferrals) */
  uint64_t host_syncs;                 /* host waits on the device inside the calls (counter reads between the merge
                                          tiers, snapshot workspace sizing, ...): one per call for a batch the lean
                                          kernels finish, two when the general tiers are needed, more for the
                                          large-document and sequential tiers */
  uint64_t docs_pending;               /* snapshots of updates that leave pending structs / a pending delete set
                                          (finished by merging [state, pendingDs, pending structs] on the GPU) */
  uint64_t docs_snapshot;              /* documents the snapshot kernels were run on (ygm_snapshot_v1, and the snapshots
                                          inside ygm_contains_v1 / ygm_sync_step2_v1 / the shared-state forms: there one
                                          per state and chunk, not one per ask; one per document of
                                          ygm_version_take_v1, two per document of ygm_version_restore_v1, one per state
                                          and chunk plus one per ask of ygm_version_restore_shared_v1, one per document
                                          of ygm_tojson_v1) */
} ygm_stats_t;

/* Opens the engine on HIP device `device` (one context per GPU; contexts are
 * independent, not thread-safe: one batch in flight per context). */
int ygm_open(int device, uint32_t flags, ygm_ctx **out);
void ygm_close(ygm_ctx *ctx);

/* ---- host-memory batch API (what the N-API addon / ctypes binding call) ---
 * arena      concatenated V1 updates
 * upd_off    n_upd+1 byte offsets into arena
 * upd_doc    n_upd document ids, non-decreasing; updates of a document keep
 *            their order (the order of yjs's `updates` array) */
int ygm_merge_v1(ygm_ctx *ctx, const uint8_t *arena, const uint64_t *upd_off, const uint32_t *upd_doc,
                 uint32_t n_upd, uint32_t n_docs, ygm_result *out);
/* doc_off: n_docs+1 offsets of one update per document; sv_off: n_docs+1
 * offsets of one encoded state vector per document in sv_arena. */
int ygm_diff_v1(ygm_ctx *ctx, const uint8_t *arena, const uint64_t *doc_off, const uint8_t *sv_arena,
                const uint64_t *sv_off, uint32_t n_docs, ygm_result *out);
int ygm_sv_from_update_v1(ygm_ctx *ctx, const uint8_t *arena, const uint64_t *doc_off, uint32_t n_docs,
                          ygm_result *out);

/* Doc-normalized snapshot: Y.encodeStateAsUpdate(Y.applyUpdate(new Y.Doc(), update)) per document
 * -- the bytes extension-database stores (packages/extension-database/src/Database.ts:55-60,
 * Y.encodeStateAsUpdate of the live document): YATA-integrated, deleted content garbage-collected,
 * adjacent structs merged (yjs Y@20500-32900 readUpdate / cleanupTransactions, Y@23300
 * encodeStateAsUpdate).  One update per document (e.g. the output of ygm_merge_v1).  An update whose
 * document keeps pending structs / a pending delete set (lost or out-of-order updates) gives yjs's bytes
 * too: mergeUpdates([state, pendingDs, pending structs]) (Y@23300), run by the merge kernels.  Sub-documents
 * (ContentDoc) are integrated like any one-clock content.  Documents outside the envelope (repeated client
 * blocks, overlapping structs) carry YGM_EUNSUPPORTED. */
int ygm_snapshot_v1(ygm_ctx *ctx, const uint8_t *arena, const uint64_t *doc_off, uint32_t n_docs, ygm_result *out);

/* ---- per-document options: documents created with gc: false -----------------
 * The reference lets a deployment switch Yjs garbage collection off, globally (yDocOptions { gc, gcFilter },
 * packages/server/src/types.ts:152-154) or per document (onCreateDocument's yDocOptions spread over the global
 * ones, packages/server/src/Hocuspocus.ts:331-344); extension-database then stores Y.encodeStateAsUpdate of that
 * live document with its deleted Items and their content (packages/extension-database/src/Database.ts:55-60).
 * The *_opts_v1 forms take one option byte per document (doc_opt / state_opt, n_docs bytes; NULL: every byte 0,
 * the forms above, byte for byte).  Bit 0 is YGM_DOC_NO_GC; a byte with any other bit set gives that document
 * YGM_EINVAL and nothing else (its neighbours are unaffected).  A gcFilter predicate cannot be expressed. */
#define YGM_DOC_NO_GC 1u   /* per-document option byte: the document is a Y.Doc({gc:false}) */
/* ygm_snapshot_v1 with options: a YGM_DOC_NO_GC document's snapshot is
 * Y.encodeStateAsUpdate(Y.applyUpdate(new Y.Doc({gc: false}), update)) -- tryGcDeleteSet does not run: deleted Items
 * keep their content (a deleted type its children), adjacent deleted String / Any / JSON Items merge with each
 * other; integration, the delete set, pending structs and the merge pass are as in ygm_snapshot_v1
 * (Hocuspocus.ts:331-344, types.ts:152-154, Database.ts:55-60). */
int ygm_snapshot_opts_v1(ygm_ctx *ctx, const uint8_t *arena, const uint64_t *doc_off, const uint8_t *doc_opt,
                         uint32_t n_docs, ygm_result *out);
/* Read-only SyncStep2: Y.snapshotContainsUpdate(Y.snapshot(doc), update) per document
 * (packages/server/src/MessageReceiver.ts:156-179; yjs 13.6 snapshotContainsUpdate).  states: each
 * document's state (any update: its Y.snapshot view -- the store's integrated part, without pending structs or
 * a pending delete set -- is taken by the snapshot kernels first; a ygm_snapshot_v1 output is its own view);
 * updates: the received update per document.  Document d's output is one byte, 1 = contained (the
 * server acks with SyncStatus true), 0 = new content (SyncStatus false). */
int ygm_contains_v1(ygm_ctx *ctx, const uint8_t *states, const uint64_t *state_off, const uint8_t *updates,
                    const uint64_t *update_off, uint32_t n_docs, ygm_result *out);
/* (ygm_contains_v1 has no options form: Y.snapshot(doc) is a state vector and a delete set, and both are the same
 * with or without garbage collection, so the answer for a gc: false document is the one above.) */
/* ---- plain text of stored documents ----------------------------------------
 * What a stored document says, without loading it into a Y.Doc: for doc = Y.applyUpdate(new Y.Doc(), state) and a
 * root name (UTF-8 bytes, compared bytewise with the root-type names in the update), document d's output is
 *   YGM_TEXT_FLAT  the UTF-8 of doc.getText(name).toString() (yjs YText.toString: from the type's _start along
 *                  right, every item that is not deleted, is countable and holds a ContentString appends its string;
 *                  embeds, formats, Any, JSON, binary, nested types and sub-documents are skipped);
 *   YGM_TEXT_DEEP  the same walk that also descends, at a live ContentType item, into that type's list and on return
 *                  appends one 0x0A unless the output is still empty or already ends in 0x0A -- the text of an
 *                  XmlFragment / Tiptap document, whose strings live in XmlText nodes below the root.  Map entries
 *                  (items with a parentSub) are on no list: attributes and Y.Map values contribute nothing.
 * A string cut through a surrogate pair by a concurrent insert or a delete carries U+FFFD on both sides, as
 * ContentString.splice leaves it.  states / state_off as ygm_snapshot_v1; names / name_off: one root name per
 * document (n_docs + 1 offsets; names may be NULL when every name is empty).  A name the update has no root for
 * gives the empty text with YGM_OK (doc.getText creates an empty type).  A state that leaves pending structs / a
 * pending delete set is read through its integrated part, as ygm_version_take_v1 reads it, with YGM_OK.  Any other
 * status is the one the state's parse and integration give in ygm_snapshot_v1 (YGM_EMALFORMED, YGM_ERANGE,
 * YGM_EUNSUPPORTED, ...) and affects only its own document.  A mode other than the two is YGM_EINVAL for the call.
 * Outputs are packed in document order.
 * (ygm_text_v1 has no options form: the text depends neither on YGM_F_COMPAT_135 nor on garbage collection -- a
 * deleted item is skipped whether or not its content was collected.)
 * (Replaces no single reference interface: the reference's server code never calls getText().toString(); this is
 * the batched form of the per-document load-and-walk a search indexer, a webhook body or a version preview does.) */
#define YGM_TEXT_FLAT 0u
#define YGM_TEXT_DEEP 1u
int ygm_text_v1(ygm_ctx *ctx, const uint8_t *states, const uint64_t *state_off, const uint8_t *names,
                const uint64_t *name_off, uint32_t mode, uint32_t n_docs, ygm_result *out);
/* ---- stored documents as ProseMirror / Tiptap JSON ---------------------------
 * What a stored document is, without loading it into a Y.Doc: for doc = Y.applyUpdate(new Y.Doc(), state) and a root
 * name (UTF-8 bytes, compared bytewise, as in ygm_text_v1), document d's output for kind YGM_JSON_PROSEMIRROR is the
 * UTF-8 of
 *     JSON.stringify(yXmlFragmentToProsemirrorJSON(doc.getXmlFragment(name)))
 * that is JSON.stringify(TiptapTransformer.fromYdoc(doc, name)) -- y-prosemirror's function (the reference pins
 * 1.3.4), restated over yjs 13.5.16's toArray / toDelta / getAttributes / nodeName:
 *     serialize(XmlText)    = toDelta().map(d => { type:'text', text:d.insert,
 *                               marks?: Object.keys(d.attributes).map(k => ({ type:k, attrs:d.attributes[k] })) })
 *     serialize(XmlElement) = { type:nodeName, attrs?: getAttributes() (when it has a key),
 *                               content?: toArray().map(serialize).flat() (when toArray() is not empty) }
 *     result                = { type:'doc', content: fragment.toArray().map(serialize) }   (top level not flattened)
 * with the keys in exactly that order.  toArray keeps a list's live countable items.  toDelta: a live ContentFormat
 * flushes the pending string, then a null value deletes its key from currentAttributes (a Map) and any other sets it
 * (an existing key keeps its place; delete then set moves it to the end); live ContentStrings append to the pending
 * string (U+FFFD on both sides of a cut surrogate pair); a live ContentEmbed flushes and gives one op whose text is
 * the embed's JSON value; the end of the list flushes; deleted items are ignored; ops with equal marks are not
 * merged, strings across deleted items are.  getAttributes: the type's map entries whose current item is not
 * deleted, the value the last element of its ContentAny.  attrs and marks follow JavaScript's own-property order:
 * canonical array-index keys ascending, then insertion order.  Any values are written as the V2 -> V1 conversion
 * writes them, format and embed values (canonical JSON text in V1) are copied, strings are escaped as JSON.stringify
 * escapes them (\" \\ \b \f \n \r \t, other bytes below 0x20 as \u00xx, everything else verbatim).
 * A name the update has no root for gives {"type":"doc","content":[]} with YGM_OK; a state with pending structs / a
 * pending delete set is read through its integrated part with YGM_OK.  Refusals affect only their own document
 * (length 0); in the asked root's subtree:
 *   a live list child of a fragment or element that is not a type; a child type that is neither XmlElement nor
 *   XmlText; a live type inside an XmlText; a live attribute that is not a ContentAny, or whose value is undefined or
 *   a Uint8Array; a mark key ending in "--" plus 8 characters of [A-Za-z0-9+/=] (newer y-prosemirror versions
 *   rewrite such names)                                                                   YGM_EUNSUPPORTED
 *   a number in an attribute, mark or embed that is not an integer JSON.stringify writes without an exponent
 *   (as ygm_convert_v2_to_v1 refuses it)                                                  YGM_ENONCANON
 *   a number of more than 15 significant digits in a mark or embed value (9007199254740992: the state's parse takes
 *   it as not canonical, as in ygm_snapshot_v1, so the refusal holds for every root name asked, an absent one
 *   included)                                                                             YGM_ENONCANON
 *   a BigInt (JSON.stringify throws)                                                      YGM_EMALFORMED
 *   a JSON of 2^31 bytes or more                                                          YGM_ENOMEM
 * Any other status is the one the state's parse and integration give in ygm_snapshot_v1.  The caller keeps its yjs
 * path for refused documents.  A JSON has no bound in its state's size (every op repeats the current marks): one
 * that does not fit its workspace is neither cut nor refused -- the documents concerned run a second time into a
 * region sized from their recorded lengths, at the cost of one more host wait (ygm_stats_t.host_syncs).
 * states / state_off / names / name_off, tail padding, packing and the other statuses as ygm_text_v1.  A kind other
 * than YGM_JSON_PROSEMIRROR is YGM_EINVAL for the call (toJSON of Map and Array roots: ygm_tojson_v1).  No options form:
 * the JSON depends neither on YGM_F_COMPAT_135 nor on garbage collection.
 * With YGM_F_FLOATS (ygm_open): the first YGM_ENONCANON row above does not apply -- an attribute's finite float32 /
 * float64 is written as Number.prototype.toString writes it, and a mark or embed value holding a non-integer number of
 * at most 15 significant digits and no exponent is copied as it stands; an attribute that is not finite (JSON.stringify
 * writes null, the conversion refuses) and the second row (more than 15 significant digits, or an exponent) stay
 * YGM_ENONCANON.
 * (Replaces packages/transformer/src/Prosemirror.ts:26: transformer.fromYdoc(document, fieldName) with one field
 * name, what a REST read of one field sends.  The body of a change webhook is ygm_json_fields_v1 below.) */
#define YGM_JSON_PROSEMIRROR 0u
int ygm_json_v1(ygm_ctx *ctx, const uint8_t *states, const uint64_t *state_off, const uint8_t *names,
                const uint64_t *name_off, uint32_t kind, uint32_t n_docs, ygm_result *out);
/* ---- every field of a stored document as one JSON object ----------------------
 * The multi-field form of ygm_json_v1: one load of the state serializes every asked root, or all roots.  For
 * doc = Y.applyUpdate(new Y.Doc(), state), document d's output is the UTF-8 of
 *     JSON.stringify(TiptapTransformer.fromYdoc(doc, fields))        fields: undefined | string[]
 * that is { "<field>": <what ygm_json_v1 gives for that field>, ... }.
 * fields / field_off hold one field list per document (n_docs + 1 offsets; fields may be NULL when every list is
 * empty).  A list is zero or more lib0 varStrings back to back, each a varuint byte length followed by UTF-8 bytes:
 *   zero bytes         every key of doc.share -- fromYdoc(document) with no field name, or with []
 *   one or more names  fromYdoc(document, [names...]); the empty name "" is a valid field
 * Key order is JavaScript's own-property order of the data[field] = ... assignments made in list order (for all
 * fields: doc.share insertion order, the order in which the state's structs first name their roots): canonical
 * array-index keys ascending, then the other keys in first-assignment order.  A name repeated in a list keeps its
 * first position and appears once.  Keys are escaped as JSON.stringify escapes strings.  A listed name the state has
 * no root for gives {"type":"doc","content":[]}; a document with no roots, asked for all fields, gives {}; a root
 * that has only map entries serializes as an empty doc; a state with pending structs / a pending delete set is read
 * through its integrated part with YGM_OK, and roots that only pending structs name are in doc.share, so they
 * appear, empty, in the all-fields form.
 * A list gives its own document YGM_EINVAL, and nothing else, when a length runs past the list's end, a varuint is
 * non-minimal or longer than 5 bytes, a name is not well-formed UTF-8 (it is written into the output), or the list
 * holds more than 1024 names.
 * Refusals leave length 0 and affect only their own document:
 *   a state's parse or integration status (as ygm_json_v1) comes before anything about the fields, its list included
 *   the refusal ygm_json_v1 gives for the first refusing field in output order (index keys ascending, then the
 *   rest; the reference throws, so the order only has to be fixed)
 *   a field named __proto__, where it stands in that order (in JavaScript the assignment sets the prototype and the
 *   key silently vanishes; the caller's yjs path reproduces that)                          YGM_EUNSUPPORTED
 *   an object of 2^31 bytes or more                                                        YGM_ENOMEM
 * The object is larger than any of its roots: the second run of ygm_json_v1 covers it in the same way.  states /
 * state_off, tail padding, packing and the other statuses as ygm_json_v1; a kind other than YGM_JSON_PROSEMIRROR is
 * YGM_EINVAL for the call.  No options form: neither YGM_F_COMPAT_135 nor garbage collection changes the result.
 * With YGM_F_FLOATS (ygm_open) every field is written as ygm_json_v1 writes it with the flag.
 * (Replaces packages/extension-webhook/src/index.ts:119 -- the `document` of every change webhook,
 * transformer.fromYdoc(data.document) -- and packages/transformer/src/Prosemirror.ts:29-39.) */
int ygm_json_fields_v1(ygm_ctx *ctx, const uint8_t *states, const uint64_t *state_off, const uint8_t *fields,
                       const uint64_t *field_off, uint32_t kind, uint32_t n_docs, ygm_result *out);
/* ---- toJSON of stored Map, Array and Text roots -------------------------------
 * What a stored document holds when it is not a rich-text document: boards, forms, whiteboards, notebook models keep
 * their state in Y.Map / Y.Array / Y.Text roots.  For doc = Y.applyUpdate(new Y.Doc(), state) and a root name (UTF-8
 * bytes, compared bytewise, as in ygm_text_v1), document d's output is the UTF-8 of
 *   YGM_TOJSON_MAP    JSON.stringify(doc.getMap(name).toJSON())
 *   YGM_TOJSON_ARRAY  JSON.stringify(doc.getArray(name).toJSON())
 *   YGM_TOJSON_TEXT   JSON.stringify(doc.getText(name).toJSON())
 * with yjs 13.5.16's toJSON.  The asked kind decides how the root is read (an update does not say what a root is); a
 * nested type is read by its typeRef (0 Array, 1 Map, 2 Text).
 *   Map    the type's map entries whose current item is not deleted; the value is the last element of the item's
 *          content.  Keys follow JavaScript's own-property order: canonical array-index keys ascending, then the
 *          order in which the keys were first set (a key set again keeps its place).  A value that is undefined drops
 *          its key.  An empty or absent root gives {}.  The root's list items are ignored.
 *   Array  the list's live countable items, every content element in turn; an undefined element is null; map entries
 *          on the same root are ignored.  An absent root gives [].
 *   Text   toString() -- YGM_TEXT_FLAT's walk: live countable ContentStrings only, U+FFFD on both sides of a cut
 *          surrogate pair -- as one JSON string.  An absent root gives "".
 * Contents: a ContentType recurses by its typeRef; every element of a ContentAny is written as below; every element
 * of a ContentJSON (canonical JSON text in V1) is copied, the word undefined counting as undefined, with the float
 * refusal ygm_json_v1 applies to embed values.  Any values are written as the V2 -> V1 conversion writes them, with two
 * additions: inside an Any an undefined object member is dropped and an undefined array element is null; a float32
 * or float64 that is not finite is null, one that is an integer of magnitude at most 2^53 is its decimal digits
 * (Date.now() timestamps and 4294967296 travel this way; negative zero is 0).  Strings and keys are escaped as in
 * ygm_json_v1.
 * Refusals affect only their own document (length 0); the state's own parse or integration status comes first, as in
 * ygm_json_v1; in the asked root's subtree:
 *   a nested XmlElement / XmlFragment / XmlHook / XmlText (typeRef 3-6: their toJSON is an XML string, not built
 *   here) or an unknown typeRef                                                           YGM_EUNSUPPORTED
 *   a ContentBinary, or a Uint8Array anywhere in an Any (JSON.stringify writes an index-keyed object)
 *                                                                                         YGM_EUNSUPPORTED
 *   a ContentDoc                                                                          YGM_EUNSUPPORTED
 *   a live ContentString or ContentEmbed in an Array's list                               YGM_EUNSUPPORTED
 *   a live Map entry that is not ContentAny / ContentJSON / ContentType                   YGM_EUNSUPPORTED
 *   a Y.Map key __proto__ with a live entry (the assignment sets the prototype and the key vanishes, as in
 *   ygm_json_fields_v1)                                                                   YGM_EUNSUPPORTED
 *   a finite non-integer number, or an integer above 2^53                                 YGM_ENONCANON
 *   a BigInt (JSON.stringify throws)                                                      YGM_EMALFORMED
 *   nesting past the walk stack                                                           YGM_ENOMEM, as ygm_json_v1
 *   a JSON of 2^31 bytes or more                                                          YGM_ENOMEM
 * A state with pending structs / a pending delete set is read through its integrated part with YGM_OK.  A JSON has no
 * bound in its state's size (a control character is written as six bytes): the second run of ygm_json_v1 covers it
 * in the same way, at the cost of one more host wait (ygm_stats_t.host_syncs).  ygm_stats_t.docs_snapshot grows by
 * n_docs.  states / state_off / names / name_off, tail padding, packing and the other statuses as ygm_json_v1.  A kind
 * other than the three is YGM_EINVAL for the call.  No options form: neither YGM_F_COMPAT_135 nor garbage collection
 * changes the result.
 * Out of scope: the shortest-round-trip decimal of non-integer doubles; XML strings of nested Xml types; toDelta; a
 * multi-root object form.
 * With YGM_F_FLOATS (ygm_open): the YGM_ENONCANON row above does not apply -- every finite float32 / float64 of an Any
 * is written as Number.prototype.toString writes it (a non-integer, an integer above 2^53; a float32 widened exactly
 * first), and a ContentJSON element holding a non-integer number of at most 15 significant digits and no exponent is
 * copied as it stands; one with more digits or an exponent stays YGM_ENONCANON by the state's parse.  A number of up
 * to 25 bytes stands where 9 stood in the state: the second run covers it.
 * (Replaces no single reference interface: the batched form of a custom webhook transformer's `fromYdoc`,
 * extension-webhook/src/index.ts:27-31,119.) */
#define YGM_TOJSON_MAP 0u   /* JSON.stringify(doc.getMap(name).toJSON())   */
#define YGM_TOJSON_ARRAY 1u /* JSON.stringify(doc.getArray(name).toJSON()) */
#define YGM_TOJSON_TEXT 2u  /* JSON.stringify(doc.getText(name).toJSON())  */
int ygm_tojson_v1(ygm_ctx *ctx, const uint8_t *states, const uint64_t *state_off, const uint8_t *names,
                  const uint64_t *name_off, uint32_t kind, uint32_t n_docs, ygm_result *out);
/* SyncStep2 payload of a stored document: Y.encodeStateAsUpdate(doc, sv) for doc = Y.applyUpdate(new Y.Doc(), state)
 * -- what the reference sends in reply to a SyncStep1 (packages/server/src/MessageReceiver.ts:137-138) for a
 * document loaded from stored bytes (extension-database Database.ts:44-50).  Computed as the doc-normalized
 * snapshot of `state` (ygm_snapshot_v1) followed by diffUpdate(snapshot, sv) in which every struct keeps its
 * parentSub bit (Item.write of an integrated item, yjs Y@80416).  states / state_off as ygm_snapshot_v1;
 * sv_arena / sv_off one encoded state vector per document.  A state that leaves pending structs / a pending delete
 * set is answered as yjs does: mergeUpdates([writeStateAsUpdate(doc, sv), pendingDs, diffUpdate(pending structs,
 * sv)]) (Y@23300; the pending structs diffed without the kept bit).  A document outside the snapshot envelope
 * carries YGM_EUNSUPPORTED (the caller names it and keeps its yjs path). */
int ygm_sync_step2_v1(ygm_ctx *ctx, const uint8_t *states, const uint64_t *state_off, const uint8_t *sv_arena,
                      const uint64_t *sv_off, uint32_t n_docs, ygm_result *out);
/* ygm_sync_step2_v1 with options: for a YGM_DOC_NO_GC state the reply is Y.encodeStateAsUpdate(doc, sv) of the
 * uncollected document, doc = Y.applyUpdate(new Y.Doc({gc: false}), state) -- the deleted Items are sent with their
 * content, as the reference's live gc: false document sends them (Hocuspocus.ts:331-344, types.ts:152-154; the stored
 * bytes of Database.ts:55-60).  Computed as diffUpdate of the no-GC snapshot with the kept parentSub bit; a state
 * that leaves pending parts takes the three-way merge, of which only the state part depends on the option. */
int ygm_sync_step2_opts_v1(ygm_ctx *ctx, const uint8_t *states, const uint64_t *state_off, const uint8_t *state_opt,
                           const uint8_t *sv_arena, const uint64_t *sv_off, uint32_t n_docs, ygm_result *out);

/* ---- version history: batched Y.snapshot and Y.createDocFromSnapshot --------
 * What gc: false is for: a version per store window, and an old version shown to a client.
 *
 * ygm_version_take_v1: Y.encodeSnapshot(Y.snapshot(doc)), doc = Y.applyUpdate(new Y.Doc(), state) -- the encoded
 * Snapshot V1: writeDeleteSet of the store's delete set, then writeStateVector.  states / state_off as
 * ygm_snapshot_v1.  A state that leaves pending structs / a pending delete set is seen through its integrated part,
 * as Y.snapshot(doc) sees the store.  The delete-set section is the one a snapshot ends with; the state vector is
 * a count and (client, next clock) pairs, in the store's insertion order under YGM_F_COMPAT_135 (13.5's
 * writeStateVector iterates the Map: clients integrated as 3 then 9 give ... 02 03 06 09 03) and client-descending
 * otherwise (13.6 sorts; like the rest of the default mode, not pinned by vectors of a 13.6 bundle).  The delete set
 * is the same with or without garbage collection, so there is no options form. */
int ygm_version_take_v1(ygm_ctx *ctx, const uint8_t *states, const uint64_t *state_off, uint32_t n_docs, ygm_result *out);
/* ygm_version_restore_v1: Y.encodeStateAsUpdate(Y.createDocFromSnapshot(doc, Y.decodeSnapshot(version), newDoc)),
 * doc = Y.applyUpdate(new Y.Doc({gc: false}), state); newDoc = new Y.Doc(), or new Y.Doc({gc: false}) when
 * restored_opt[d] has YGM_DOC_NO_GC (restored_opt: n_docs bytes or NULL; a byte with any other bit gives that
 * document YGM_EINVAL and nothing else).  versions / version_off: one encoded Snapshot V1 per document.  Computed as
 * the no-GC snapshot S of the state's integrated part, the cut of S at the version's clocks followed by the version's
 * delete set (one parse: a straddled Item's content is shortened as ContentX.splice does, U+FFFD for a cut surrogate
 * pair in both modes; a straddled GC struct stays whole, yjs splits only Items), and the snapshot of that update into
 * newDoc.  A version that is not causally closed, or whose delete set reaches past the kept clocks, leaves pending
 * parts there, answered as ygm_snapshot_v1 answers them.  A state's refusal (YGM_EUNSUPPORTED, YGM_EMALFORMED, ...)
 * is the document's status.  Per document, the version gives:
 *   truncated version                                              YGM_EMALFORMED
 *   a varuint above 2^53                                           YGM_ERANGE
 *   a non-minimal varuint in the version                           YGM_ENONCANON
 *   a client repeated in its delete set or in its state vector     YGM_ENONCANON  (yjs would re-encode;
 *                                                                  Y.encodeSnapshot never writes these)
 *   a version clock above the state's clock for that client        YGM_EINVAL     (yjs throws)
 *   a version client with clock > 0 that the state does not have   YGM_EINVAL     (yjs throws)
 *   more than 4096 state-vector entries (or delete-set clients),
 *   a client id past 32 bits                                       YGM_EUNSUPPORTED
 * Bytes after the state vector are ignored, as decodeSnapshot ignores them.  Each refusal affects only its own
 * document.  To restore several versions of one document, use ygm_version_restore_shared_v1 below: the pair form
 * stages and snapshots the state once per version. */
int ygm_version_restore_v1(ygm_ctx *ctx, const uint8_t *states, const uint64_t *state_off, const uint8_t *versions,
                           const uint64_t *version_off, const uint8_t *restored_opt, uint32_t n_docs, ygm_result *out);

/* ---- shared-state forms: many state vectors answered from one state ---------
 * A reconnect storm sends many SyncStep1 messages for one document.  These forms take n_docs states and n_asks
 * state vectors; ask_doc[a] (ask_state[a]) names the state that ask a is answered from.  The result has one entry
 * per ask, in ask order (out->n_docs == n_asks), each byte-identical to what ygm_diff_v1 / ygm_sync_step2_v1 return
 * for the pair (state[ask_doc[a]], sv[a]); each state is uploaded once, snapshotted once (step2), and read by the
 * diff kernels in place.
 *   doc_off / state_off   n_docs + 1 offsets of one update per state
 *   sv_off                n_asks + 1 offsets of one encoded state vector per ask
 *   ask_doc / ask_state   n_asks state ids, non-decreasing (the convention of upd_doc in ygm_merge_v1), each
 *                         below n_docs; a state may have no ask
 * An unordered or out-of-range id gives YGM_EINVAL before any device work.  A state's refusal (YGM_EUNSUPPORTED,
 * YGM_EMALFORMED, ...) is the status of each of its asks; a bad state vector fails only its own ask.
 * Chunks are ranges of states together with their asks, cut by virtual bytes (a chunk's state bytes plus, over its
 * asks, the ask's state length: what bounds the output slots).  One state whose asks alone exceed the chunk budget
 * is split over several chunks, and each of those chunks stages and snapshots that state again: a split state costs
 * one snapshot per chunk, not per ask. */
int ygm_diff_shared_v1(ygm_ctx *ctx, const uint8_t *arena, const uint64_t *doc_off, uint32_t n_docs,
                       const uint8_t *sv_arena, const uint64_t *sv_off, const uint32_t *ask_doc, uint32_t n_asks,
                       ygm_result *out);
int ygm_sync_step2_shared_v1(ygm_ctx *ctx, const uint8_t *states, const uint64_t *state_off, uint32_t n_states,
                             const uint8_t *sv_arena, const uint64_t *sv_off, const uint32_t *ask_state, uint32_t n_asks,
                             ygm_result *out);
/* ygm_sync_step2_shared_v1 with options: state_opt holds one byte per state (n_states), and every ask of a state is
 * answered from that state's snapshot, so from its option (Hocuspocus.ts:331-344, types.ts:152-154,
 * Database.ts:55-60); a bad byte's YGM_EINVAL is the status of each of the state's asks.  A state split over several
 * chunks carries its byte into each of them. */
int ygm_sync_step2_shared_opts_v1(ygm_ctx *ctx, const uint8_t *states, const uint64_t *state_off, const uint8_t *state_opt,
                                  uint32_t n_states, const uint8_t *sv_arena, const uint64_t *sv_off,
                                  const uint32_t *ask_state, uint32_t n_asks, ygm_result *out);
/* ygm_version_restore_v1 over shared states: many versions restored from one stored state (a history sidebar, a
 * scrubber, an export of every version of a document).  n_states states, n_asks versions, ask_state[a] naming the
 * state that version a is restored from, under the rules of ask_state above.  One result per ask, in ask order
 * (out->n_docs == n_asks), each byte-identical, with identical status, to what ygm_version_restore_v1 returns for the
 * pair (state[ask_state[a]], version[a], restored_opt[a]), in both modes.  Each state is staged once and given its
 * no-GC snapshot once; the cut reads that snapshot in place for every ask; only the restored documents are
 * snapshotted per ask.  restored_opt holds one byte per ask (n_asks bytes, or NULL): the option belongs to the new
 * document, not to the state; a byte with any bit other than YGM_DOC_NO_GC gives that ask YGM_EINVAL and nothing
 * else.  A state's refusal is the status of each of its asks; a bad version fails only its own ask, by the table
 * under ygm_version_restore_v1.  Chunks are cut as for ygm_sync_step2_shared_v1: a split state is staged and
 * snapshotted once per chunk, and a chunk stages its asks' option bytes. */
int ygm_version_restore_shared_v1(ygm_ctx *ctx, const uint8_t *states, const uint64_t *state_off, uint32_t n_states,
                                  const uint8_t *versions, const uint64_t *version_off, const uint32_t *ask_state,
                                  const uint8_t *restored_opt, uint32_t n_asks, ygm_result *out);

/* ---- update format V2 ------------------------------------
 * The same operations over yjs's column-encoded update format V2 (UpdateEncoderV2 / UpdateDecoderV2,
 * yjs Y@15400-18900; lib0 RLE column coders), used by yjs providers other than Hocuspocus's V1 path:
 *   ygm_merge_v2            <- Y.mergeUpdatesV2(updates)                 (yjs Y@39011, V2 coders)
 *   ygm_diff_v2             <- Y.diffUpdateV2(update, stateVector)       (yjs Y@40711)
 *   ygm_sv_from_update_v2   <- Y.encodeStateVectorFromUpdateV2(update)   (yjs Y@37728; V1 state vector out)
 *   ygm_convert_v1_to_v2    <- Y.convertUpdateFormatV1ToV2(update)       (yjs 13.6)
 *   ygm_convert_v2_to_v1    <- Y.convertUpdateFormatV2ToV1(update)       (yjs 13.6)
 * Arguments as the V1 forms.  The conversions take updates in the lazy writer's normal form (what every
 * yjs encoder writes) and refuse others with YGM_ENONCANON, as they refuse V2 -> V1 of embed / format values
 * holding non-integer numbers (their JSON.stringify decimal is not reproduced).  mergeUpdatesV2 of one
 * update returns it as it is, as yjs does. */
int ygm_merge_v2(ygm_ctx *ctx, const uint8_t *arena, const uint64_t *upd_off, const uint32_t *upd_doc,
                 uint32_t n_upd, uint32_t n_docs, ygm_result *out);
int ygm_diff_v2(ygm_ctx *ctx, const uint8_t *arena, const uint64_t *doc_off, const uint8_t *sv_arena,
                const uint64_t *sv_off, uint32_t n_docs, ygm_result *out);
int ygm_sv_from_update_v2(ygm_ctx *ctx, const uint8_t *arena, const uint64_t *doc_off, uint32_t n_docs,
                          ygm_result *out);
int ygm_convert_v1_to_v2(ygm_ctx *ctx, const uint8_t *arena, const uint64_t *doc_off, uint32_t n_docs, ygm_result *out);
int ygm_convert_v2_to_v1(ygm_ctx *ctx, const uint8_t *arena, const uint64_t *doc_off, uint32_t n_docs, ygm_result *out);

/* ---- device-resident API (inputs already in HBM; used by bench.py) --------
 * All pointers are device pointers.  doc_upd: n_docs+1 update-index offsets
 * (document d owns updates doc_upd[d] .. doc_upd[d+1]); upd_off must be
 * non-decreasing.  Results stay on the device: the data/off/len/status
 * pointers of the result point into context-owned device memory.  Outputs
 * are NOT packed: document d's bytes are data[off[d] .. off[d]+len[d]) inside
 * its own slot (2*in_off + 64*d, capacity 2*|in| + 64) or, for documents the
 * lean kernels defer, in a region after the slots (merge: overflow cursor;
 * SV / diff: packed by the exact per-document kernel); data_bytes is the used
 * extent of `data`, payload_bytes the sum of len[].  `stream` is a
 * hipStream_t (NULL = the context's stream); the call returns after one
 * read of the launch counters.
 * Tail padding: the kernels read inputs in aligned 16-byte pieces and 64-byte chunks, so at least
 * 64 readable bytes must follow d_arena + arena_bytes and the end of d_sv_arena (zeroed or not: they
 * are never taken as input).  The host API pads its own staging copies. */
typedef struct {
  uint8_t *data;
  uint64_t *off;
  uint64_t *len;
  int32_t *status;
  uint64_t data_bytes;
  uint64_t payload_bytes;
} ygm_device_result;

int ygm_merge_v1_device(ygm_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_upd_off,
                        const uint32_t *d_doc_upd, uint32_t n_upd, uint32_t n_docs, void *stream,
                        ygm_device_result *out);
/* Asynchronous form of ygm_merge_v1_device for GPU-resident pipelines: enqueues
 * the counter reset and the lean kernel on `stream` and returns without waiting.
 * Documents the lean kernel finishes are complete when the stream reaches this
 * point; every other document (deferred to the wave / workgroup / sequential
 * tiers) is completed by ygm_merge_v1_device_finish, which waits for the stream,
 * runs the tiers the device counters ask for, checks the fault flag and fills
 * out->data_bytes / payload_bytes.  A context holds one batch: the next enqueue
 * on it reuses the result buffers.
 * (Replaces no single reference interface: the batched form of Y.mergeUpdates,
 * yjs Y@37704, for GPU-resident pipelines.) */
int ygm_merge_v1_device_async(ygm_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_upd_off,
                              const uint32_t *d_doc_upd, uint32_t n_upd, uint32_t n_docs, void *stream);
int ygm_merge_v1_device_finish(ygm_ctx *ctx, ygm_device_result *out);
/* Compact input form of ygm_merge_v1_device(_async): the documents' updates are contiguous in the arena, so
 * d_doc_off[d] (u64, n_docs + 1 entries) is the byte offset of document d's first update, d_doc_off[n_docs] the
 * end of the last, and d_upd_len[i] (u16, n_upd entries) the byte length of update i (every update < 64 KiB; a
 * batch with a larger one takes the u64 form).  2 bytes per update instead of 8 -- for a log of one-character
 * inserts the table is a third of the input bytes -- and no u64 table at all unless a document leaves the lean
 * kernel (the context then builds its entries on the device).  Lengths that do not add up to the document's bytes
 * give that document YGM_EMALFORMED (yjs reading past an update's end throws).  Results, finish and reuse as ygm_merge_v1_device(_async).
 * (Replaces no single reference interface: the batched form of Y.mergeUpdates, yjs Y@37704.) */
int ygm_merge_v1_device_lens(ygm_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_doc_off,
                             const uint16_t *d_upd_len, const uint32_t *d_doc_upd, uint32_t n_upd, uint32_t n_docs, void *stream,
                             ygm_device_result *out);
int ygm_merge_v1_device_lens_async(ygm_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_doc_off,
                                   const uint16_t *d_upd_len, const uint32_t *d_doc_upd, uint32_t n_upd, uint32_t n_docs,
                                   void *stream);
int ygm_diff_v1_device(ygm_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_doc_off,
                       const uint8_t *d_sv_arena, const uint64_t *d_sv_off, uint32_t n_docs, void *stream,
                       ygm_device_result *out);
int ygm_sv_from_update_v1_device(ygm_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes,
                                 const uint64_t *d_doc_off, uint32_t n_docs, void *stream,
                                 ygm_device_result *out);

int ygm_snapshot_v1_device(ygm_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_doc_off,
                           uint32_t n_docs, void *stream, ygm_device_result *out);
/* Device-resident options forms: d_doc_opt / d_state_opt are device pointers to the option bytes (one per document
 * or state; NULL: none set), as doc_opt / state_opt of the host forms (Hocuspocus.ts:331-344, types.ts:152-154,
 * Database.ts:55-60). */
int ygm_snapshot_opts_v1_device(ygm_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_doc_off,
                                const uint8_t *d_doc_opt, uint32_t n_docs, void *stream, ygm_device_result *out);

int ygm_contains_v1_device(ygm_ctx *ctx, const uint8_t *d_states, const uint64_t *d_state_off, const uint8_t *d_updates,
                           const uint64_t *d_update_off, uint32_t n_docs, void *stream, ygm_device_result *out);
/* ygm_text_v1, device-resident, as ygm_snapshot_v1_device: 64 readable bytes must follow both arenas, results are
 * not packed (a flat-text document asked by its root name has its text in its slot, align16(2 * d_state_off[d] +
 * 64 * d); any other in the workspace region after the slots), payload_bytes is the sum of the lengths.
 * (Replaces no single reference interface, as ygm_text_v1.) */
int ygm_text_v1_device(ygm_ctx *ctx, const uint8_t *d_states, uint64_t states_bytes, const uint64_t *d_state_off,
                       const uint8_t *d_names, const uint64_t *d_name_off, uint32_t mode, uint32_t n_docs, void *stream,
                       ygm_device_result *out);
/* ygm_json_v1, device-resident, as ygm_text_v1_device: 64 readable bytes must follow both arenas, results are not
 * packed (a document's JSON lies in its workspace's output region, or in the overflow region after the workspaces
 * when it ran a second time), payload_bytes is the sum of the lengths.
 * (Replaces packages/transformer/src/Prosemirror.ts:26, as ygm_json_v1.) */
int ygm_json_v1_device(ygm_ctx *ctx, const uint8_t *d_states, uint64_t states_bytes, const uint64_t *d_state_off,
                       const uint8_t *d_names, const uint64_t *d_name_off, uint32_t kind, uint32_t n_docs, void *stream,
                       ygm_device_result *out);
/* ygm_json_fields_v1, device-resident: tail padding, the unpacked result and payload_bytes as ygm_json_v1_device; a
 * field list may start at any byte of its arena.
 * (Replaces packages/extension-webhook/src/index.ts:119, packages/transformer/src/Prosemirror.ts:29-39.) */
int ygm_json_fields_v1_device(ygm_ctx *ctx, const uint8_t *d_states, uint64_t states_bytes, const uint64_t *d_state_off,
                              const uint8_t *d_fields, const uint64_t *d_field_off, uint32_t kind, uint32_t n_docs,
                              void *stream, ygm_device_result *out);
/* ygm_tojson_v1, device-resident: tail padding, the unpacked result (a document's JSON lies in its workspace's output
 * region, or in the overflow region after the workspaces when it ran a second time) and payload_bytes as
 * ygm_json_v1_device.
 * (Replaces no single reference interface, as ygm_tojson_v1.) */
int ygm_tojson_v1_device(ygm_ctx *ctx, const uint8_t *d_states, uint64_t states_bytes, const uint64_t *d_state_off,
                         const uint8_t *d_names, const uint64_t *d_name_off, uint32_t kind, uint32_t n_docs, void *stream,
                         ygm_device_result *out);
int ygm_sync_step2_v1_device(ygm_ctx *ctx, const uint8_t *d_states, uint64_t states_bytes, const uint64_t *d_state_off,
                             const uint8_t *d_sv_arena, const uint64_t *d_sv_off, uint32_t n_docs, void *stream,
                             ygm_device_result *out);
int ygm_sync_step2_opts_v1_device(ygm_ctx *ctx, const uint8_t *d_states, uint64_t states_bytes, const uint64_t *d_state_off,
                                  const uint8_t *d_state_opt, const uint8_t *d_sv_arena, const uint64_t *d_sv_off,
                                  uint32_t n_docs, void *stream, ygm_device_result *out);

/* Version history, device-resident (ygm_version_take_v1 / ygm_version_restore_v1 above): two arenas as
 * ygm_contains_v1_device, option bytes as ygm_snapshot_opts_v1_device (d_restored_opt NULL: none set).  The cut kernel
 * reads aligned 16-byte pieces: d_versions must be 16-byte aligned (YGM_EINVAL otherwise) and, like d_states, be
 * followed by 64 readable bytes. */
int ygm_version_take_v1_device(ygm_ctx *ctx, const uint8_t *d_states, uint64_t states_bytes, const uint64_t *d_state_off,
                               uint32_t n_docs, void *stream, ygm_device_result *out);
int ygm_version_restore_v1_device(ygm_ctx *ctx, const uint8_t *d_states, const uint64_t *d_state_off,
                                  const uint8_t *d_versions, const uint64_t *d_version_off, const uint8_t *d_restored_opt,
                                  uint32_t n_docs, void *stream, ygm_device_result *out);

/* Shared-state forms, device-resident: d_ask_doc (u32, n_asks entries) as ask_doc above; d_sv_off has n_asks + 1
 * entries; results are indexed by ask.  Ask a's slot is placed from the exclusive scan, over asks, of each ask's
 * state length (2 * ask_base[a] + 64 * a).  An id that is out of range or below its predecessor is never used as an
 * index: that ask carries YGM_EINVAL. */
int ygm_diff_shared_v1_device(ygm_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_doc_off,
                              uint32_t n_docs, const uint8_t *d_sv_arena, const uint64_t *d_sv_off,
                              const uint32_t *d_ask_doc, uint32_t n_asks, void *stream, ygm_device_result *out);
int ygm_sync_step2_shared_v1_device(ygm_ctx *ctx, const uint8_t *d_states, uint64_t states_bytes,
                                    const uint64_t *d_state_off, uint32_t n_states, const uint8_t *d_sv_arena,
                                    const uint64_t *d_sv_off, const uint32_t *d_ask_state, uint32_t n_asks, void *stream,
                                    ygm_device_result *out);
int ygm_sync_step2_shared_opts_v1_device(ygm_ctx *ctx, const uint8_t *d_states, uint64_t states_bytes,
                                         const uint64_t *d_state_off, const uint8_t *d_state_opt, uint32_t n_states,
                                         const uint8_t *d_sv_arena, const uint64_t *d_sv_off, const uint32_t *d_ask_state,
                                         uint32_t n_asks, void *stream, ygm_device_result *out);
/* ygm_version_restore_shared_v1, device-resident: d_version_off has n_asks + 1 entries, d_restored_opt n_asks bytes
 * (NULL: none set).  The ask plan runs over the packed no-GC snapshots: ask a's cut goes to the slot
 * al16(ask_base[a] + d_version_off[a] + 32 * a), ask_base the exclusive scan, over asks, of the ask's snapshot
 * length.  As in the pair form, d_versions must be 16-byte aligned (YGM_EINVAL otherwise) and both arenas be followed
 * by 64 readable bytes.  ygm_stats_t.docs_snapshot grows by n_states + n_asks. */
int ygm_version_restore_shared_v1_device(ygm_ctx *ctx, const uint8_t *d_states, uint64_t states_bytes,
                                         const uint64_t *d_state_off, uint32_t n_states, const uint8_t *d_versions,
                                         const uint64_t *d_version_off, const uint32_t *d_ask_state,
                                         const uint8_t *d_restored_opt, uint32_t n_asks, void *stream,
                                         ygm_device_result *out);

/* update V2, device-resident (outputs packed in document order: off[d] increasing) */
int ygm_merge_v2_device(ygm_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_upd_off,
                        const uint32_t *d_doc_upd, uint32_t n_upd, uint32_t n_docs, void *stream, ygm_device_result *out);
int ygm_diff_v2_device(ygm_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_doc_off,
                       const uint8_t *d_sv_arena, const uint64_t *d_sv_off, uint32_t n_docs, void *stream,
                       ygm_device_result *out);
int ygm_sv_from_update_v2_device(ygm_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes,
                                 const uint64_t *d_doc_off, uint32_t n_docs, void *stream, ygm_device_result *out);
int ygm_convert_v1_to_v2_device(ygm_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_doc_off,
                                uint32_t n_docs, void *stream, ygm_device_result *out);
int ygm_convert_v2_to_v1_device(ygm_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_doc_off,
                                uint32_t n_docs, void *stream, ygm_device_result *out);

int ygm_stats(ygm_ctx *ctx, ygm_stats_t *out);
const char *ygm_strerror(int code);
const char *ygm_version(void);

#ifdef __cplusplus
}
#endif
#endif /* YGM_H */
