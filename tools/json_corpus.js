'use strict'
// ProseMirror-JSON corpus for ygm_json_v1 (test tooling): what a stored document is, as y-prosemirror's
// yXmlFragmentToProsemirrorJSON (TiptapTransformer.fromYdoc(doc, name)) serializes it.  y-prosemirror itself is not
// available to this tool: `serialize` below restates its function over yjs's own toArray / toDelta / getAttributes /
// nodeName, and the yjs is 13.5.16 (the image's bundle, tools/yjs_bundle.js) -- the same pinning as the deep-text
// walker of tools/text_corpus.js.
// For every state of five committed snapshot fixtures (the `u` of each row) the state is applied to a fresh Y.Doc; for
// every root name in doc.share and for one absent name the tool records [nameHex, status, jsonHex]: status 0 with
//   json = utf8(JSON.stringify({ type: 'doc', content: doc.getXmlFragment(name).toArray().map(serialize) }))
// or a refusal of include/ygm.h's table (9 YGM_EUNSUPPORTED, 3 YGM_ENONCANON, 1 YGM_EMALFORMED for a BigInt) with no
// bytes.  Rows past the first FULL of a set keep [nameHex, status, sha256(json), length] instead.  The states are not
// stored again (row i belongs to row i of the input fixture, whose sha256 is recorded); the edge sessions are
// generated here by yjs and carry their own states.
//   node tools/json_corpus.js <out.json.gz> [limit]     (limit: only the first `limit` states of each set)
//   node tools/json_corpus.js --states <in.json> <out.json.gz>     (given states and the boundary sessions: see statesMode)
const fs = require('fs')
const path = require('path')
const zlib = require('zlib')
const crypto = require('crypto')
const Y = require(path.join(__dirname, 'yjs_bundle.js')).load()

const GOLDEN = path.join(__dirname, '..', 'tests', 'golden')
const SETS = ['snapshot_v135', 'snapshot_text_v135', 'snapshot_pending_v135', 'snapshot_subdoc_v135', 'snapshot_nogc_v135']
const ABSENT = 'no-such-root'
const FULL = 40
const HASHED = /--[A-Za-z0-9+/=]{8}$/

const ContentAny = (() => {   // the content constructor, from a document of the bundle's own
  const d = new Y.Doc()
  const e = new Y.XmlElement('p')
  d.getXmlFragment('f').insert(0, [e])
  e.setAttribute('k', 'v')
  return e._map.get('k').content.constructor
})()

class Refuse extends Error { constructor (st) { super('refused ' + st); this.st = st } }
// the refusal table of a context opened with YGM_F_FLOATS (tools/floats_corpus.js turns it on; this tool's own fixtures
// are made with it off)
let FLOATS = false
const setFloats = on => { FLOATS = !!on }

// a value that came from JSON text (a format or embed value): numbers JSON.stringify writes as plain integers of at
// most 15 significant digits (more are not canonical to the engine's JSON check, as in the snapshot)
const sigDigits = v => String(Math.abs(v)).replace(/^0\./, '').replace(/\./, '').replace(/^0+/, '').replace(/0+$/, '').length
function checkJson (v) {
  if (typeof v === 'number') { if ((!FLOATS && !Number.isInteger(v)) || /e/.test(String(v)) || sigDigits(v) > 15) throw new Refuse(3) } else if (Array.isArray(v)) v.forEach(checkJson)
  else if (v !== null && typeof v === 'object') Object.keys(v).forEach(k => checkJson(v[k]))
}
// a value that came from an Any (an attribute): what the engine's Any -> JSON conversion writes
function checkAny (v) {
  if (typeof v === 'bigint') throw new Refuse(1)
  if (typeof v === 'number') { if (FLOATS ? !Number.isFinite(v) : (!Number.isInteger(v) || Math.abs(v) > 2147483647)) throw new Refuse(3) } else if (v === undefined || v instanceof Uint8Array) throw new Refuse(3)
  else if (Array.isArray(v)) v.forEach(checkAny)
  else if (v !== null && typeof v === 'object') Object.keys(v).forEach(k => checkAny(v[k]))
}

function serialize (item) {
  if (item !== null && item !== undefined && item.constructor === Y.XmlText) {
    return item.toDelta().map(d => {
      if (d.insert !== null && typeof d.insert === 'object' && typeof d.insert.toDelta === 'function') throw new Refuse(9)   // a type in a text
      if (d.insert !== null && typeof d.insert === 'object' && d.insert._item !== undefined) throw new Refuse(9)
      const text = { type: 'text', text: d.insert }
      if (typeof d.insert !== 'string') checkJson(d.insert)
      if (d.attributes) {
        text.marks = Object.keys(d.attributes).map(k => {
          if (HASHED.test(k)) throw new Refuse(9)
          checkJson(d.attributes[k])
          return { type: k, attrs: d.attributes[k] }
        })
      }
      return text
    })
  }
  if (item !== null && item !== undefined && item.constructor === Y.XmlElement) {
    const r = { type: item.nodeName }
    item._map.forEach(it => {
      if (it.deleted) return
      if (it.content.constructor !== ContentAny) throw new Refuse(9)
      const v = it.content.getContent()[it.length - 1]
      if (v === undefined || v instanceof Uint8Array) throw new Refuse(9)
      checkAny(v)
    })
    const attrs = item.getAttributes()
    if (Object.keys(attrs).length) r.attrs = attrs
    const children = item.toArray()
    if (children.length) r.content = children.map(serialize).flat()
    return r
  }
  throw new Refuse(9)   // a list child that is no type, or a type that is neither XmlElement nor XmlText
}

function jsonOf (doc, name) {
  return JSON.stringify({ type: 'doc', content: doc.getXmlFragment(name).toArray().map(serialize) })
}

// What the state's parse refuses whatever root is asked (include/ygm.h: "any other status is the one the state's
// parse and integration give in ygm_snapshot_v1"), as far as the sessions of this tool reach it: YGM_ENONCANON for a
// format or embed value holding a number JSON.stringify writes with an exponent or with more than 15 significant
// digits, and for an Any integer below -2147483647 (13.5's writeAny stores it as a varint no Y.Doc writes back).
function stateRefusal (doc) {
  let st = 0
  const json = v => {
    if (typeof v === 'number') { if (Number.isFinite(v) && (/e/.test(String(v)) || sigDigits(v) > 15)) st = 3 } else if (Array.isArray(v)) v.forEach(json)
    else if (v !== null && typeof v === 'object') Object.keys(v).forEach(k => json(v[k]))
  }
  const any = v => {
    if (typeof v === 'number') { if (Number.isInteger(v) && v < -2147483647) st = 3 } else if (Array.isArray(v)) v.forEach(any)
    else if (v !== null && typeof v === 'object' && !(v instanceof Uint8Array)) Object.keys(v).forEach(k => any(v[k]))
  }
  doc.store.clients.forEach(structs => structs.forEach(it => {
    if (it.content === undefined) return   // (a GC struct)
    const ref = it.content.getRef()
    if (ref === 6) json(it.content.value)
    else if (ref === 5) json(it.content.embed)
    else if (ref === 8) it.content.arr.forEach(any)
  }))
  return st
}

// [[nameHex, status, json (utf8 string)], ...] for the state's roots (doc.share order) and the absent name
function rootsOf (state) {
  const probe = new Y.Doc()
  Y.applyUpdate(probe, state)
  const names = Array.from(probe.share.keys())
  names.push(ABSENT)
  const whole = stateRefusal(probe)
  return names.map(name => {
    if (whole) return [Buffer.from(name, 'utf8').toString('hex'), whole, '']
    const doc = new Y.Doc()   // (a fresh document per ask: getXmlFragment fixes a root's type)
    Y.applyUpdate(doc, state)
    try {
      return [Buffer.from(name, 'utf8').toString('hex'), 0, jsonOf(doc, name)]
    } catch (e) {
      if (!(e instanceof Refuse)) throw e
      return [Buffer.from(name, 'utf8').toString('hex'), e.st, '']
    }
  })
}
const fullRow = r => [r[0], r[1], Buffer.from(r[2], 'utf8').toString('hex')]
const hashRow = r => { const b = Buffer.from(r[2], 'utf8'); return [r[0], r[1], crypto.createHash('sha256').update(b).digest('hex'), b.length] }

// ---- sessions: [note, state]
const frag = d => d.getXmlFragment('default')
const el = (parent, at, nodeName) => { const e = new Y.XmlElement(nodeName); parent.insert(at, [e]); return e }
const txt = (parent, at, s, attrs) => { const t = new Y.XmlText(); parent.insert(at, [t]); if (s !== null) t.insert(0, s, attrs); return t }
const para = (parent, at, s) => { const e = el(parent, at, 'paragraph'); if (s !== null) txt(e, 0, s); return e }

function edges () {
  const out = []
  const one = (note, id, f) => { const d = new Y.Doc(); d.clientID = id; f(d); out.push([note, Y.encodeStateAsUpdate(d)]) }
  // structure
  one('an empty fragment', 101, d => { const f = frag(d); para(f, 0, 'x'); f.delete(0, 1) })
  one('an XmlText directly under the fragment', 102, d => { const f = frag(d); txt(f, 0, 'top'); para(f, 1, 'after'); txt(f, 2, 'again') })
  one('a paragraph without children', 103, d => { para(frag(d), 0, null) })
  one('a paragraph with an empty XmlText', 104, d => { txt(el(frag(d), 0, 'paragraph'), 0, null) })
  one('a paragraph whose children are all deleted', 105, d => { const e = para(frag(d), 0, 'gone'); para(e, 1, 'also'); e.delete(0, 2) })
  one('a deleted subtree between two live ones', 106, d => { const f = frag(d); para(f, 0, 'keep-a'); const e = para(f, 1, 'gone'); para(e, 1, 'gone-child'); para(f, 2, 'keep-b'); f.delete(1, 1) })
  one('nesting 40 deep', 107, d => {
    let p = frag(d)
    for (let i = 0; i < 40; i++) { const e = el(p, 0, 'n' + i); if (i % 7 === 3) txt(e, 0, 'L' + i); if (i % 11 === 5) e.setAttribute('depth', i); p = e }
    txt(p, p.length, 'bottom')
  })
  // attrs
  one('attrs: a key set twice', 111, d => { const e = para(frag(d), 0, 'x'); e.setAttribute('a', 'one'); e.setAttribute('b', 'two'); e.setAttribute('a', 'three') })
  one('attrs: a key set then deleted, alone', 112, d => { const e = para(frag(d), 0, 'x'); e.setAttribute('a', 'one'); e.removeAttribute('a') })
  one('attrs: a key set then deleted beside a live one', 113, d => { const e = para(frag(d), 0, 'x'); e.setAttribute('a', 'one'); e.setAttribute('b', 'two'); e.removeAttribute('a') })
  one('attrs: keys "10", "9", "a", "04" set in that order', 114, d => { const e = para(frag(d), 0, 'x'); for (const k of ['10', '9', 'a', '04']) e.setAttribute(k, 'v' + k) })
  {
    const a = new Y.Doc(); a.clientID = 115
    const b = new Y.Doc(); b.clientID = 116
    const e = para(frag(a), 0, 'x'); e.setAttribute('first', 'f')
    Y.applyUpdate(b, Y.encodeStateAsUpdate(a))
    e.setAttribute('k', 'from-a'); frag(b).get(0).setAttribute('k', 'from-b'); frag(b).get(0).setAttribute('only-b', 1)
    Y.applyUpdate(a, Y.encodeStateAsUpdate(b))
    out.push(['attrs: two clients setting one key concurrently', Y.encodeStateAsUpdate(a)])
  }
  one('attrs: values of every kind', 117, d => {
    const e = el(frag(d), 0, 'heading')
    e.setAttribute('s', 'q" b\\ \b\f\n\r\t \u0001\u001f \u007f \u2028 😀')
    e.setAttribute('n', -42); e.setAttribute('t', true); e.setAttribute('f', false); e.setAttribute('z', null)
    e.setAttribute('o', { k: [1, 'two', { deep: null }], '2': 'index', e: {} }); e.setAttribute('arr', [[], {}, 0])
  })
  one('refused: a string child in an element list', 121, d => { const e = para(frag(d), 0, 'x'); e.insert(1, ['plain']) })
  one('refused: a Y.Map child (typeRef 1)', 122, d => { const f = frag(d); para(f, 0, 'x'); f.insert(1, [new Y.Map()]) })
  one('refused: a type inside an XmlText', 123, d => { const t = txt(para(frag(d), 0, null), 0, 'ab'); t.insertEmbed(1, new Y.XmlElement('inline')) })
  one('refused: an attribute that is a Uint8Array (ContentBinary)', 124, d => { para(frag(d), 0, 'x').setAttribute('bin', new Uint8Array([1, 2, 3])) })
  one('refused: an attribute that is undefined', 125, d => { para(frag(d), 0, 'x').setAttribute('u', undefined) })
  one('refused: an attribute that is a nested type', 126, d => { para(frag(d), 0, 'x').setAttribute('t', new Y.XmlText()) })
  one('refused: a hashed mark name', 127, d => { txt(para(frag(d), 0, null), 0, 'marked', { 'comment--AbCd012+': { id: 7 } }) })
  one('refused: a float attribute', 128, d => { para(frag(d), 0, 'x').setAttribute('w', 1.5) })
  one('refused: a float in a mark', 129, d => { txt(para(frag(d), 0, null), 0, 'marked', { size: { pt: 10.5 } }) })
  one('refused: a float in an embed', 130, d => { txt(para(frag(d), 0, null), 0, 'ab').insertEmbed(1, { ratio: 0.5 }) })
  if (typeof BigInt === 'function') one('refused: a BigInt in an attribute', 131, d => { para(frag(d), 0, 'x').setAttribute('big', { n: BigInt(5) }) })
  // marks
  one('marks: on then off', 141, d => { const t = txt(para(frag(d), 0, null), 0, 'plain bold plain'); t.format(6, 4, { bold: true }) })
  one('marks: two marks, one re-set in place, one removed and re-added', 142, d => {
    const t = txt(para(frag(d), 0, null), 0, 'aaaabbbbccccdddd')
    t.format(0, 16, { bold: true }); t.format(0, 16, { italic: true })
    t.format(4, 12, { bold: { v: 2 } })             // bold re-set: keeps its place before italic
    t.format(8, 8, { bold: null }); t.format(12, 4, { bold: true })   // removed, re-added: after italic
  })
  {   // two clients make overlapping ranges bold, their updates merged as updates (no document ever cleans the formats
      // up): the second client's format item stands between the strings and changes nothing
    const a = new Y.Doc(); a.clientID = 143
    const b = new Y.Doc(); b.clientID = 144
    const log = []
    a.on('update', (u, o, doc, tr) => { if (tr.local) log.push(u) })
    b.on('update', (u, o, doc, tr) => { if (tr.local) log.push(u) })
    txt(para(frag(a), 0, null), 0, 'onetwo')
    Y.applyUpdate(b, Y.encodeStateAsUpdate(a))
    frag(a).get(0).get(0).format(3, 3, { bold: true })
    frag(b).get(0).get(0).format(0, 6, { bold: true })
    out.push(['marks: the same value set twice between strings (two ops with equal marks)', Y.mergeUpdates(log)])
  }
  one('marks: a deleted format item', 144, d => { const t = txt(para(frag(d), 0, null), 0, 'abcdef'); t.format(2, 2, { em: true }); t.format(2, 2, { em: null }) })
  one('marks: a format at the end of the list', 145, d => { const t = txt(para(frag(d), 0, null), 0, 'tail', { bold: true }); t.insert(4, 'x', { bold: true, code: true }); t.delete(4, 1) })
  one('marks: across an embed', 146, d => { const t = txt(para(frag(d), 0, null), 0, 'before after', { link: { href: 'https://example.org/?a="b"' } }); t.insertEmbed(6, { image: 'x.png', w: 3 }, { link: { href: 'https://example.org/?a="b"' } }); t.insertEmbed(0, { rule: true }) })
  one('marks: index-like mark keys', 147, d => { txt(para(frag(d), 0, null), 0, 'keys', { b: true, '10': 'ten', '9': 'nine', '04': 'text', a: 1 }) })
  one('marks: values true, {}, a string, an object', 148, d => { const t = txt(para(frag(d), 0, null), 0, 'abcd'); t.format(0, 1, { a: true }); t.format(1, 1, { b: {} }); t.format(2, 1, { c: 'str "q"' }); t.format(3, 1, { d: { x: [1, null], y: { z: false } } }) })
  one('marks: a deleted string between two strings under equal marks (one op)', 149, d => { const t = txt(para(frag(d), 0, null), 0, 'left', { bold: true }); t.insert(4, 'MID', { bold: true }); t.insert(7, 'right', { bold: true }); t.delete(4, 3) })
  // strings
  one('strings: every escape class', 151, d => { txt(para(frag(d), 0, null), 0, 'q" b\\ \b\f\n\r\t \u0001\u001f \u007f \u2028 😀 end') })
  {
    const a = new Y.Doc(); a.clientID = 152
    const b = new Y.Doc(); b.clientID = 153
    txt(para(frag(a), 0, null), 0, 'a😀b')
    Y.applyUpdate(b, Y.encodeStateAsUpdate(a))
    frag(b).get(0).get(0).insert(2, 'X')
    frag(a).get(0).get(0).insert(4, 'tail')
    Y.applyUpdate(a, Y.encodeStateAsUpdate(b))
    out.push(['strings: an emoji split by a concurrent insert', Y.encodeStateAsUpdate(a)])
  }
  one('strings: a node name and an attribute key that contain a quote', 154, d => { const e = el(frag(d), 0, 'no"de\\'); e.setAttribute('k"e\ny', 'v'); txt(e, 0, 'x') })
  {   // state: two peers typing, then a lost update (pending structs with an integrated part)
    const a = new Y.Doc(); a.clientID = 161
    const b = new Y.Doc(); b.clientID = 162
    const log = []
    a.on('update', (u, o, doc, tr) => { if (tr.local) log.push(u) })
    b.on('update', (u, o, doc, tr) => { if (tr.local) log.push(u) })
    const e = para(frag(a), 0, 'shared ')
    e.setAttribute('level', 1)
    Y.applyUpdate(b, Y.encodeStateAsUpdate(a))
    e.get(0).insert(7, 'from-a')
    frag(b).get(0).get(0).insert(7, 'from-b', { bold: true })
    Y.applyUpdate(a, Y.encodeStateAsUpdate(b)); Y.applyUpdate(b, Y.encodeStateAsUpdate(a))
    para(frag(a), 1, 'second')
    frag(a).get(1).get(0).insert(6, ' more')
    const lost = log.slice(); lost.splice(lost.length - 2, 1)
    out.push(['state: pending structs with an integrated part', Y.mergeUpdates(lost)])
  }
  // overflow: every op repeats every mark set so far
  one('overflow: 64 one-character strings, each under one more mark', 171, d => {
    const t = txt(para(frag(d), 0, null), 0, null)
    const attrs = {}
    for (let i = 0; i < 64; i++) { attrs['mark-number-' + i] = { n: i, s: 'value-' + i }; t.insert(i, String.fromCharCode(65 + (i % 26)), Object.assign({}, attrs)) }
  })
  return out
}

// ---- boundary sessions (tests/golden/json_overflow_v135.json.gz): keys at the edge of an array index, mark names
// around the hashed form, numbers at the edge of what is written, XmlTexts and refused types between siblings
const INDEX_KEYS = ['4294967295', '4294967294', '0', '00', '-1', '4294967296', '12345678901', '1.0', '7']
function boundary () {
  const out = []
  const one = (note, id, f) => { const d = new Y.Doc(); d.clientID = id; f(d); out.push([note, Y.encodeStateAsUpdate(d)]) }
  one('index keys as attributes: ' + INDEX_KEYS.join(' '), 201, d => { const e = para(frag(d), 0, 'x'); for (const k of INDEX_KEYS) e.setAttribute(k, 'v' + k) })
  one('index keys as marks, set one by one: ' + INDEX_KEYS.join(' '), 202, d => { const t = txt(para(frag(d), 0, null), 0, 'keys'); for (const k of INDEX_KEYS) t.format(0, 4, { [k]: 'v' + k }) })
  let id = 210
  for (const k of ['--AbCd0123', '-AbCd0123x', 'c--AbCd012', 'c--AbCd01_2', 'c--AbCd0123x', 'é--AbCd0123', 'c--========']) {
    one('mark name ' + k, id++, d => { txt(para(frag(d), 0, null), 0, 'marked', { [k]: { id: 7 } }) })
  }
  {   // a hashed mark set and nulled around a string that is deleted by a delete set alone (no document cleans the
      // formats up): the mark is never current at a string, so it is never written
    const a = new Y.Doc(); a.clientID = 120
    const b = new Y.Doc(); b.clientID = 121
    txt(para(frag(a), 0, null), 0, 'tail')
    const ua = Y.encodeStateAsUpdate(a)
    Y.applyUpdate(b, ua)
    let ub = null
    b.on('update', u => { ub = u })
    frag(b).get(0).get(0).insert(0, 'x', { 'c--AbCd0123': true })   // clocks of 121: format 0, 'x' 1, format (null) 2
    out.push(['a hashed mark set and nulled before any live string', Y.mergeUpdates([ua, ub, Uint8Array.from([0, 1, 121, 1, 1, 1])])])
  }
  for (const v of [2147483647, -2147483647, 2147483648, -2147483648, 0, -0]) {
    one('attribute integer ' + (Object.is(v, -0) ? '-0' : String(v)), id++, d => { para(frag(d), 0, 'x').setAttribute('n', v) })
  }
  one('mark numbers 1e20, -0, 123456789012', id++, d => { txt(para(frag(d), 0, null), 0, 'nums', { a: 1e20, b: { z: -0 }, c: [123456789012] }) })
  one('mark number 1e21', id++, d => { txt(para(frag(d), 0, null), 0, 'nums', { a: 1e21 }) })
  one('a mark key and string values that hold digits, dots and e', id++, d => { txt(para(frag(d), 0, null), 0, 'strs', { '1.5e3': '2.5e10', k: { '1e5': '-3.14', 'e.1': ['0.5', 'e'] } }) })
  one('mark number of 16 digits', id++, d => { txt(para(frag(d), 0, null), 0, 'nums', { big: { v: 9007199254740992 } }) })
  one('four XmlTexts in one element: the first ends bold, one is empty, then an element, then text', id++, d => {
    const e = el(frag(d), 0, 'paragraph')
    txt(e, 0, 'ends-bold', { bold: true }); txt(e, 1, null); txt(e, 2, 'plain')
    txt(el(e, 3, 'inner'), 0, 'inside'); txt(e, 4, 'last')
  })
  one('empty XmlTexts directly under the fragment, between elements', id++, d => {
    const f = frag(d)
    txt(f, 0, null); para(f, 1, 'a'); txt(f, 2, null); txt(f, 3, null); para(f, 4, 'b'); txt(f, 5, null)
  })
  one('embed values {} and an array', id++, d => { const t = txt(para(frag(d), 0, null), 0, 'abc'); t.insertEmbed(1, {}); t.insertEmbed(3, [1, [2, 'x'], {}], { bold: true }) })
  one('refused: a nested XmlFragment child', id++, d => { const f = frag(d); para(f, 0, 'x'); f.insert(1, [new Y.XmlFragment()]) })
  one('refused: an XmlHook child', id++, d => { const f = frag(d); para(f, 0, 'x'); f.insert(1, [new Y.XmlHook('hook')]) })
  one('refused: a Y.Text child', id++, d => { const f = frag(d); para(f, 0, 'x'); f.insert(1, [new Y.Text('plain')]) })
  return out
}

// --states <in.json> <out.json.gz>: in.json is { source, states: [hex] }; the output holds rootsOf of every state (its
// roots and the absent name; a JSON of more than HASH_OVER bytes as [nameHex, status, sha256, length]) and the
// boundary sessions with their states.  Driven by tools/json_overflow_fixture.py.
const HASH_OVER = 4096
const sizedRow = r => Buffer.byteLength(r[2], 'utf8') > HASH_OVER ? hashRow(r) : fullRow(r)
function statesMode (inFile, outFile) {
  const inp = JSON.parse(fs.readFileSync(inFile, 'utf8'))
  const doc = {
    source: inp.source,
    absent: Buffer.from(ABSENT, 'utf8').toString('hex'),
    hash_over: HASH_OVER,
    states: inp.states.map(h => rootsOf(Buffer.from(h, 'hex')).map(sizedRow)),
    sessions: boundary().map(([note, state]) => ({ note, state: Buffer.from(state).toString('hex'), roots: rootsOf(state).map(sizedRow) }))
  }
  fs.writeFileSync(outFile, zlib.gzipSync(Buffer.from(JSON.stringify(doc)), { level: 9 }))
  console.log(JSON.stringify({ states: doc.states.length, sessions: doc.sessions.length }))
}

// --time <asks.bin>: the CPU path this replaces, on one core: per ask (tools/snapdev/jsondev.cpp's input: state, root
// name) a fresh Y.Doc, applyUpdate, the serializer, JSON.stringify.  One JSON line.
function timeAsks (file, lo, hi) {
  const b = fs.readFileSync(file)
  const n = b.readUInt32LE(0)
  const asks = []
  let p = 4
  for (let i = 0; i < n; i++) {
    const sl = b.readUInt32LE(p); const state = b.subarray(p + 4, p + 4 + sl); p += 4 + sl
    const nl = b.readUInt32LE(p); const name = b.subarray(p + 4, p + 4 + nl).toString('utf8'); p += 4 + nl
    if (i >= lo && i < hi) asks.push([state, name])
  }
  let best = Infinity; let bytes = 0; let refused = 0
  for (let rep = 0; rep < 3; rep++) {
    bytes = 0; refused = 0
    const t0 = process.hrtime.bigint()
    for (const [state, name] of asks) {
      const doc = new Y.Doc()
      Y.applyUpdate(doc, state)
      try { bytes += Buffer.byteLength(jsonOf(doc, name), 'utf8') } catch (e) { if (!(e instanceof Refuse)) throw e; refused++ }
    }
    best = Math.min(best, Number(process.hrtime.bigint() - t0) / 1e6)
  }
  console.log(JSON.stringify({ asks: asks.length, json_bytes: bytes, refused, yjs_ms: Math.round(best * 100) / 100 }))
}

if (require.main === module && process.argv[2] === '--time') {
  timeAsks(process.argv[3], process.argv[4] ? parseInt(process.argv[4], 10) : 0, process.argv[5] ? parseInt(process.argv[5], 10) : Infinity)
} else if (require.main === module && process.argv[2] === '--states') {
  statesMode(process.argv[3], process.argv[4])
} else if (require.main === module) {
  const limit = process.argv[3] ? parseInt(process.argv[3], 10) : Infinity
  const inputs = {}
  const sets = {}
  const counts = {}
  for (const s of SETS) {
    const raw = fs.readFileSync(path.join(GOLDEN, s + '.json.gz'))
    inputs[s + '.json.gz'] = crypto.createHash('sha256').update(raw).digest('hex')
    const rows = JSON.parse(zlib.gunzipSync(raw).toString()).rows
    const c = { states: 0, roots: 0, ok: 0, refused: 0, marks: 0, attrs: 0 }
    sets[s] = rows.slice(0, limit).map((r, i) => {
      const x = rootsOf(Buffer.from(r[0], 'hex'))
      c.states++
      for (const q of x.slice(0, -1)) {
        c.roots++
        if (q[1] === 0) { c.ok++; if (q[2].includes('"marks":[')) c.marks++; if (q[2].includes('"attrs":{')) c.attrs++ } else c.refused++
      }
      return x.map(i < FULL ? fullRow : hashRow)
    })
    counts[s] = c
  }
  const edge = edges().map(([note, state]) => ({ note, state: Buffer.from(state).toString('hex'), roots: rootsOf(state).map(fullRow) }))
  const doc = {
    source: 'tools/json_corpus.js (yjs 13.5.16 bundle; y-prosemirror restated): node tools/json_corpus.js tests/golden/json_v135.json.gz',
    absent: Buffer.from(ABSENT, 'utf8').toString('hex'),
    full: FULL,
    inputs,
    counts,
    sets,
    edges: edge
  }
  fs.writeFileSync(process.argv[2], zlib.gzipSync(Buffer.from(JSON.stringify(doc)), { level: 9 }))
  // the overflow session against its workspace's output region (snap::caps_of: n + 48 (3 S + 2 D + 4) + 16 (C + 1) + 64)
  const ovf = edge[edge.length - 1]
  const od = new Y.Doc(); Y.applyUpdate(od, Buffer.from(ovf.state, 'hex'))
  let S = 0; let D = 0
  od.store.clients.forEach(structs => { S += structs.length })
  Y.createDeleteSetFromStructStore(od.store).clients.forEach(ranges => { D += ranges.length })
  const capsOut = ovf.state.length / 2 + 48 * (3 * S + 2 * D + 4) + 16 * (od.store.clients.size + 1) + 64
  console.log(JSON.stringify({ counts, edges: edge.length, overflow_state_bytes: ovf.state.length / 2, overflow_caps_out: capsOut, overflow_json_bytes: ovf.roots[0][2].length / 2 }))
}

module.exports = { serialize, jsonOf, rootsOf, Refuse, setFloats, edges }
